// BatchMPC<OCP> of user-registered OCPs (device code in libuser_ocp.so, tests/cpp/user_ocp.hip): the batch is created through
// device_binding<OCP>::mpc_create (pmpc_mpc_batch_create_user), and step / solution / solution_u_at / shift / dispatch_longest_first / update
// serve it as they serve a built-in batch. Every comparison is between two device computations of the same problem, so it is bit for bit.
// Without a GPU the binary exits 77 (there is no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <polympc/polympc.hpp>

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("  EXPECT_TRUE failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++failures; } } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

using namespace polympc;

struct UserRobot { double q = 1.0; };          // must match the layout of the struct registered in user_ocp.hip
struct Pendulum {};
using ApproxA = polympc::Spline<polympc::Chebyshev<6>, 1>;
using RobotOCP = polympc::models::MobileRobot<ApproxA>;
POLYMPC_FORWARD_DECLARATION(UserRobotOCP, 3, 2, 0, 1, 0, double)
class UserRobotOCP : public polympc::ContinuousOCP<UserRobotOCP, ApproxA, polympc::DENSE> {
public:
    UserRobot device_model() const { return UserRobot(); }
};
POLYMPC_FORWARD_DECLARATION(PendulumOCP, 2, 1, 0, 1, 1, double)
class PendulumOCP : public polympc::ContinuousOCP<PendulumOCP, polympc::Spline<polympc::Chebyshev<5>, 2>, polympc::DENSE> {
public:
    Pendulum device_model() const { return Pendulum(); }
};
POLYMPC_USE_REGISTERED_OCP(UserRobotOCP, UserRobot)
POLYMPC_USE_REGISTERED_OCP(PendulumOCP, Pendulum)

static const double DT = 0.05;
static bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

// explicit Euler on the unicycle, wheel base d
static void robot_plant(std::vector<double>& s, const std::vector<double>& u, double d) {
    for (size_t b = 0; b < s.size() / 3; ++b) {
        const double v = u[2 * b], phi = u[2 * b + 1], th = s[3 * b + 2];
        s[3 * b] += DT * v * std::cos(th) * std::cos(phi); s[3 * b + 1] += DT * v * std::sin(th) * std::cos(phi); s[3 * b + 2] += DT * v * std::sin(phi) / d;
    }
}

template <class mpc_t> static void robot_setup(mpc_t& mpc, int B, double d) {
    mpc.settings().max_iter = 10; mpc.settings().line_search_max_iter = 10;
    mpc.set_time_limits(0, 2);
    Vector<2> lbu, ubu; lbu(0) = -1.5; lbu(1) = -0.75; ubu(0) = 1.5; ubu(1) = 0.75;
    Vector<1> p; p(0) = d;
    for (int b = 0; b < B; ++b) { mpc.control_bounds(b, lbu, ubu); mpc.set_static_parameters(b, p); }
}
static std::vector<double> robot_states(int B) {
    std::vector<double> x0((size_t)B * 3);
    for (int b = 0; b < B; ++b) { x0[3 * b] = 0.5 + 0.06 * b; x0[3 * b + 1] = 0.5 - 0.04 * b; x0[3 * b + 2] = 0.5 - 0.03 * (b % 3); }
    return x0;
}

// the registered robot restates the built-in one: closed loop, sampled control, shifted warm start, longest-first dispatch on the registered batch only
static void RegisteredBatchMPCMatchesBuiltin() {
    std::printf("RegisteredBatchMPCMatchesBuiltin\n");
    const int B = 9;
    BatchMPC<UserRobotOCP> user(B); BatchMPC<RobotOCP> builtin(B);
    EXPECT_EQ(user.update(), PMPC_ERR_INVALID_ARGUMENT);   // nothing resident before the first step
    robot_setup(user, B, 2.0); robot_setup(builtin, B, 2.0);
    std::vector<double> x0 = robot_states(B), ua(B * 2), ub(B * 2), xa, xb, sa, sb;
    int iters_first = 0, iters_last = 0;
    for (int k = 0; k < 5; ++k) {
        if (k == 1) EXPECT_EQ(user.dispatch_longest_first(true), PMPC_OK);   // changes the order in which the controllers start, and no result
        EXPECT_EQ(user.step(x0.data(), ua.data()), PMPC_OK);
        EXPECT_EQ(builtin.step(x0.data(), ub.data()), PMPC_OK);
        EXPECT_TRUE(same(ua, ub));
        for (int b = 0; b < B; ++b) EXPECT_TRUE(std::memcmp(&user.info(b), &builtin.info(b), sizeof(pmpc_sqp_info)) == 0);
        EXPECT_EQ(user.solution(xa), PMPC_OK); EXPECT_EQ(builtin.solution(xb), PMPC_OK);
        EXPECT_TRUE(same(xa, xb));
        EXPECT_EQ(user.solution_u_at(0.3, sa), PMPC_OK); EXPECT_EQ(builtin.solution_u_at(0.3, sb), PMPC_OK);
        EXPECT_TRUE(same(sa, sb));
        EXPECT_EQ(user.solution_u_at(0.0, sa), PMPC_OK);
        EXPECT_TRUE(same(sa, ua));   // one segment: the interpolant at t_start is the node value
        for (int b = 0; b < B; ++b) {
            if (k == 0) { iters_first += user.info(b).iter; EXPECT_TRUE(user.info(b).iter >= 2 && (ua[2 * b] != 0.0 || ua[2 * b + 1] != 0.0)); }   // a real solve
            if (k == 4) iters_last += user.info(b).iter;
        }
        EXPECT_EQ(user.shift(DT, k % 2 == 1), PMPC_OK); EXPECT_EQ(builtin.shift(DT, k % 2 == 1), PMPC_OK);
        EXPECT_EQ(user.solution(xa), PMPC_OK); EXPECT_EQ(builtin.solution(xb), PMPC_OK);
        EXPECT_TRUE(same(xa, xb));
        robot_plant(x0, ua, 2.0);
    }
    std::printf("  SQP iterations of the batch: first step %d, fifth step %d\n", iters_first, iters_last);
}

// a shape no built-in OCP has (NX = 2, NU = 1, ND = 1, NG = 1, two segments): the batch against single controllers stepped one by one
static void PendulumBatchMPCMatchesSingleControllers() {
    std::printf("PendulumBatchMPCMatchesSingleControllers\n");
    const int B = 3;
    using mpc_t = MPC<PendulumOCP>;
    BatchMPC<PendulumOCP> batch(B);
    std::vector<mpc_t> one(B);
    batch.settings().max_iter = 10; batch.settings().line_search_max_iter = 10; batch.set_time_limits(0, 2);
    Vector<1> lbu, ubu, lbg, ubg, p; lbu(0) = -3.0; ubu(0) = 3.0; lbg(0) = -1.0; ubg(0) = 1.0; p(0) = 1.0;
    for (int b = 0; b < B; ++b) {
        batch.control_bounds(b, lbu, ubu); batch.constraints_bounds(b, lbg, ubg); batch.set_static_parameters(b, p);
        one[b].settings().max_iter = 10; one[b].settings().line_search_max_iter = 10; one[b].set_time_limits(0, 2);
        one[b].control_bounds(lbu, ubu); one[b].constraints_bounds(lbg, ubg); one[b].set_static_parameters(p);
    }
    std::vector<double> x0 = {-0.8, 0.5, 0.1, -0.2, 0.8, -0.5}, u0(B), xs;
    for (int k = 0; k < 4; ++k) {
        EXPECT_EQ(batch.step(x0.data(), u0.data()), PMPC_OK);
        EXPECT_EQ(batch.solution(xs), PMPC_OK);
        for (int b = 0; b < B; ++b) {
            mpc_t::state_t s; s(0) = x0[2 * b]; s(1) = x0[2 * b + 1];
            one[b].initial_conditions(s);
            one[b].solve();
            EXPECT_EQ(one[b].info().iter, batch.info(b).iter);
            const double u = one[b].solution_u_at(0)(0);
            EXPECT_TRUE(std::memcmp(&u, &u0[b], sizeof(double)) == 0);
            EXPECT_TRUE(std::memcmp(one[b].solver().primal_solution().data(), &xs[(size_t)b * mpc_t::var_size], sizeof(double) * mpc_t::var_size) == 0);
            if (k == 0) EXPECT_TRUE(batch.info(b).iter >= 2 && u0[b] != 0.0);
        }
        for (int b = 0; b < B; ++b) {   // explicit Euler on the pendulum, d = 1
            const double th = x0[2 * b], om = x0[2 * b + 1];
            x0[2 * b] = th + DT * om; x0[2 * b + 1] = om + DT * (-9.81 * std::sin(th) - 0.1 * om + u0[b]);
        }
    }
    std::vector<double> us;
    EXPECT_EQ(batch.solution_u_at(0.7, us), PMPC_OK);   // sampled with the batch's own np / ng (no model id to ask)
    EXPECT_EQ(us.size(), (size_t)B);
    EXPECT_EQ(batch.shift(DT, true), PMPC_OK);
}

// set_static_parameters after the first step: ignored without update() (as before), in force after it — the single controller's setter acts at once
static void UpdateUploadsTheSetters() {
    std::printf("UpdateUploadsTheSetters\n");
    const int B = 3;
    using mpc_t = MPC<UserRobotOCP>;
    BatchMPC<UserRobotOCP> updated(B), stale(B), untouched(B);
    std::vector<mpc_t> one(B);
    robot_setup(updated, B, 2.0); robot_setup(stale, B, 2.0); robot_setup(untouched, B, 2.0);
    mpc_t::control_t lbu, ubu; lbu(0) = -1.5; lbu(1) = -0.75; ubu(0) = 1.5; ubu(1) = 0.75;
    mpc_t::static_param p; p(0) = 2.0;
    for (int b = 0; b < B; ++b) {
        one[b].settings().max_iter = 10; one[b].settings().line_search_max_iter = 10; one[b].set_time_limits(0, 2);
        one[b].control_bounds(lbu, ubu); one[b].set_static_parameters(p);
    }
    std::vector<double> x0 = robot_states(B), uu(B * 2), us(B * 2), un(B * 2);
    auto step_all = [&]() {
        EXPECT_EQ(updated.step(x0.data(), uu.data()), PMPC_OK); EXPECT_EQ(stale.step(x0.data(), us.data()), PMPC_OK);
        EXPECT_EQ(untouched.step(x0.data(), un.data()), PMPC_OK);
        for (int b = 0; b < B; ++b) {
            mpc_t::state_t s; s(0) = x0[3 * b]; s(1) = x0[3 * b + 1]; s(2) = x0[3 * b + 2];
            one[b].initial_conditions(s); one[b].solve();
        }
    };
    auto equals_single = [&](const std::vector<double>& u) {
        bool eq = true;
        for (int b = 0; b < B; ++b) { const auto v = one[b].solution_u_at(0); eq = eq && std::memcmp(&u[2 * b], v.data(), 2 * sizeof(double)) == 0; }
        return eq;
    };
    step_all();
    EXPECT_TRUE(same(uu, un) && same(us, un) && equals_single(uu));
    robot_plant(x0, un, 2.0);
    p(0) = 1.2;   // a shorter wheel base from now on
    Vector<1> pb; pb(0) = 1.2;
    for (int b = 0; b < B; ++b) { updated.set_static_parameters(b, pb); stale.set_static_parameters(b, pb); one[b].set_static_parameters(p); }
    EXPECT_EQ(updated.update(), PMPC_OK);
    step_all();
    EXPECT_TRUE(same(us, un));        // without update() the setter changes nothing on the device
    EXPECT_TRUE(!same(uu, un));       // with it the new parameter is in force
    EXPECT_TRUE(equals_single(uu));   // and gives what the single controller gives, whose setter acts at once
    EXPECT_TRUE(!equals_single(un));
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    RegisteredBatchMPCMatchesBuiltin();
    PendulumBatchMPCMatchesSingleControllers();
    UpdateUploadsTheSetters();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
