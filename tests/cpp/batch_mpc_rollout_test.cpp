// BatchMPC<OCP>::set_plant / rollout / plant_step (pmpc_mpc_batch_set_plant, pmpc_mpc_batch_rollout, pmpc_plant_step_batch[_user]): the closed loop
// enqueued as a whole against the same loop driven from the host over step() + plant_step(), for a built-in OCP and for registered ones, whose
// plant symbol the mirror binds weakly. Every comparison is between two device computations of the same problem, so it is bit for bit.
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

// the loop rollout() enqueues, driven from the host: [shift;] step(); plant_step() — into the rollout's layouts
template <class mpc_t>
static void host_loop(mpc_t& mpc, int B, int K, std::vector<double> x, int shift, const std::vector<double>* w, std::vector<double>& xs, std::vector<double>& us,
                      std::vector<pmpc_sqp_info>& info) {
    constexpr int nx = mpc_t::nx, nu = mpc_t::nu;
    xs.assign((size_t)B * (K + 1) * nx, 0.0); us.assign((size_t)B * K * nu, 0.0); info.resize((size_t)B * K);
    std::vector<double> u((size_t)B * nu), wk((size_t)B * nx);
    for (int k = 0; k <= K; ++k) {
        for (int b = 0; b < B; ++b) std::memcpy(&xs[((size_t)b * (K + 1) + k) * nx], &x[(size_t)b * nx], nx * sizeof(double));
        if (k == K) break;
        if (k > 0 && shift) EXPECT_EQ(mpc.shift(DT, shift == 2), PMPC_OK);
        EXPECT_EQ(mpc.step(x.data(), u.data()), PMPC_OK);
        for (int b = 0; b < B; ++b) { std::memcpy(&us[((size_t)b * K + k) * nu], &u[(size_t)b * nu], nu * sizeof(double)); info[(size_t)b * K + k] = mpc.info(b); }
        if (w) for (int b = 0; b < B; ++b) std::memcpy(&wk[(size_t)b * nx], &(*w)[((size_t)b * K + k) * nx], nx * sizeof(double));
        EXPECT_EQ(mpc.plant_step(x.data(), u.data(), DT, w ? wk.data() : nullptr), PMPC_OK);
    }
}

static void RolloutMatchesTheHostDrivenLoop() {
    std::printf("RolloutMatchesTheHostDrivenLoop\n");
    const int B = 9, K = 4;
    BatchMPC<RobotOCP> dev(B), host(B);
    BatchMPC<UserRobotOCP> user(B);
    robot_setup(dev, B, 2.0); robot_setup(host, B, 2.0); robot_setup(user, B, 2.0);
    const std::vector<double> x0 = robot_states(B);
    std::vector<double> xs, us, hxs, hus, uxs, uus, w((size_t)B * K * 3), dplant(B);
    std::vector<pmpc_sqp_info> info, hinfo;
    for (size_t i = 0; i < w.size(); ++i) w[i] = 1e-3 * std::sin(0.7 * (double)i);
    for (int b = 0; b < B; ++b) dplant[b] = 1.9 + 0.02 * b;   // the plant's wheel base differs from the controller's

    EXPECT_EQ(dev.rollout(x0.data(), K, DT, xs, us), PMPC_ERR_INVALID_ARGUMENT);   // no plant yet
    std::vector<double> s = x0, u((size_t)B * 2, 0.1);
    EXPECT_EQ(dev.plant_step(s.data(), u.data(), DT), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_TRUE(same(s, x0));
    pmpc_plant_settings ps = BatchMPC<RobotOCP>::plant_settings_default();
    EXPECT_TRUE(ps.integrator == 1 && ps.substeps == 1 && ps.control == 0);
    ps.substeps = 0;
    EXPECT_EQ(dev.set_plant(ps), PMPC_ERR_INVALID_ARGUMENT);
    ps.substeps = 2;
    EXPECT_EQ(dev.set_plant(ps, dplant.data()), PMPC_OK); EXPECT_EQ(host.set_plant(ps, dplant.data()), PMPC_OK);
    EXPECT_EQ(user.set_plant(ps, dplant.data()), PMPC_OK);   // through the weak symbol of libuser_ocp.so
    EXPECT_EQ(dev.rollout(x0.data(), 0, DT, xs, us), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_EQ(dev.rollout(x0.data(), K, -DT, xs, us), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_EQ(dev.rollout(x0.data(), K, DT, xs, us, 3), PMPC_ERR_INVALID_ARGUMENT);

    EXPECT_EQ(dev.rollout(x0.data(), K, DT, xs, us, 2, w.data(), &info), PMPC_OK);
    host_loop(host, B, K, x0, 2, &w, hxs, hus, hinfo);
    EXPECT_TRUE(same(xs, hxs)); EXPECT_TRUE(same(us, hus));
    EXPECT_TRUE(info.size() == hinfo.size() && std::memcmp(info.data(), hinfo.data(), info.size() * sizeof(pmpc_sqp_info)) == 0);
    for (int b = 0; b < B; ++b) EXPECT_TRUE(std::memcmp(&dev.info(b), &hinfo[(size_t)b * K + K - 1], sizeof(pmpc_sqp_info)) == 0);
    std::vector<double> ia, ib;
    EXPECT_EQ(dev.solution(ia), PMPC_OK); EXPECT_EQ(host.solution(ib), PMPC_OK);
    EXPECT_TRUE(same(ia, ib));
    bool moved = false, real = true;
    for (int b = 0; b < B; ++b) { moved = moved || xs[((size_t)b * (K + 1) + K) * 3] != x0[3 * b]; real = real && info[(size_t)b * K].iter >= 2; }
    EXPECT_TRUE(moved && real);
    // the registered robot restates the built-in one: the same closed loop, bit for bit
    EXPECT_EQ(user.rollout(x0.data(), K, DT, uxs, uus, 2, w.data()), PMPC_OK);
    EXPECT_TRUE(same(uxs, xs)); EXPECT_TRUE(same(uus, us));
    // a second rollout continues from the warm start the first one left, like the loop does
    EXPECT_EQ(dev.rollout(x0.data(), 2, DT, xs, us, 1), PMPC_OK);
    host_loop(host, B, 2, x0, 1, nullptr, hxs, hus, hinfo);
    EXPECT_TRUE(same(xs, hxs)); EXPECT_TRUE(same(us, hus));
}

// a shape no built-in OCP has, two segments, the control read from the iterate's interpolant
static void PendulumRolloutWithInterpolatedControl() {
    std::printf("PendulumRolloutWithInterpolatedControl\n");
    const int B = 3, K = 3;
    BatchMPC<PendulumOCP> dev(B), host(B);
    for (BatchMPC<PendulumOCP>* m : {&dev, &host}) {
        m->settings().max_iter = 10; m->settings().line_search_max_iter = 10; m->set_time_limits(0, 2);
        Vector<1> lbu, ubu, lbg, ubg, p; lbu(0) = -3.0; ubu(0) = 3.0; lbg(0) = -1.0; ubg(0) = 1.0; p(0) = 1.0;
        for (int b = 0; b < B; ++b) { m->control_bounds(b, lbu, ubu); m->constraints_bounds(b, lbg, ubg); m->set_static_parameters(b, p); }
        pmpc_plant_settings ps = BatchMPC<PendulumOCP>::plant_settings_default();
        ps.control = 1; ps.substeps = 3;
        EXPECT_EQ(m->set_plant(ps), PMPC_OK);
    }
    const std::vector<double> x0 = {-0.8, 0.5, 0.1, -0.2, 0.8, -0.5};
    std::vector<double> xs, us, hxs, hus;
    std::vector<pmpc_sqp_info> info, hinfo;
    EXPECT_EQ(dev.dispatch_longest_first(true), PMPC_OK);   // changes the order in which the controllers start, and no result
    EXPECT_EQ(dev.rollout(x0.data(), K, DT, xs, us, 1, nullptr, &info), PMPC_OK);
    host_loop(host, B, K, x0, 1, nullptr, hxs, hus, hinfo);
    EXPECT_TRUE(same(xs, hxs)); EXPECT_TRUE(same(us, hus));
    EXPECT_TRUE(std::memcmp(info.data(), hinfo.data(), info.size() * sizeof(pmpc_sqp_info)) == 0);
    for (int b = 0; b < B; ++b) EXPECT_TRUE(info[(size_t)b * K].iter >= 2 && us[(size_t)b * K] != 0.0 && xs[((size_t)b * (K + 1) + 1) * 2] != x0[2 * b]);
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    RolloutMatchesTheHostDrivenLoop();
    PendulumRolloutWithInterpolatedControl();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
