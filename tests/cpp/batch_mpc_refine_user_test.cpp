// The refine members of the C++ mirror on a REGISTERED OCP (pmpc_mpc_batch_set_lineariser, pmpc_sqp_refine_batch_user): BatchMPC<UserRobotOCP> after
// enable_refine(), BatchSolver<UserRobotOCP>::refine and Solver<UserRobotOCP>::refine against their twins on the built-in robot, which UserRobot of
// user_ocp.hip restates — gain, info and iterate bit for bit. Without enable_refine() the batch keeps refusing. Without a GPU the binary exits 77.
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
using ApproxA = polympc::Spline<polympc::Chebyshev<6>, 1>;
using RobotOCP = polympc::models::MobileRobot<ApproxA>;
POLYMPC_FORWARD_DECLARATION(UserRobotOCP, 3, 2, 0, 1, 0, double)
class UserRobotOCP : public polympc::ContinuousOCP<UserRobotOCP, ApproxA, polympc::DENSE> {
public:
    UserRobot device_model() const { return UserRobot(); }
};
POLYMPC_USE_REGISTERED_OCP(UserRobotOCP, UserRobot)

static const int NN = 7, NX = 3, NU = 2, N = 35;

template <class mpc_t> static void setup(mpc_t& mpc, int B) {
    mpc.set_time_limits(0, 2);
    Vector<2> lbu, ubu; lbu(0) = -0.6; lbu(1) = -0.3; ubu(0) = 0.6; ubu(1) = 0.3;   // tight enough for active control bounds
    Vector<1> p; p(0) = 2.0;
    for (int b = 0; b < B; ++b) { mpc.control_bounds(b, lbu, ubu); mpc.set_static_parameters(b, p); }
}
static std::vector<double> states(int B) {
    std::vector<double> x0((size_t)B * NX);
    for (int b = 0; b < B; ++b) { x0[3 * b] = 0.5 + 0.04 * b; x0[3 * b + 1] = 0.5 - 0.03 * b; x0[3 * b + 2] = 0.5 - 0.05 * (b % 3); }
    return x0;
}
template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}
template <class bs_t> static void setup_solver(bs_t& bs, int B, const std::vector<double>& x0) {
    bs.get_problem().set_time_limits(0, 2);
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < NN; ++k) { bs.lower_bound_x(b)[NX * NN + NU * k] = -0.6; bs.upper_bound_x(b)[NX * NN + NU * k] = 0.6;
                                       bs.lower_bound_x(b)[NX * NN + NU * k + 1] = -0.3; bs.upper_bound_x(b)[NX * NN + NU * k + 1] = 0.3; }
        for (int j = 0; j < NX; ++j) bs.lower_bound_x(b)[NX * NN - NX + j] = bs.upper_bound_x(b)[NX * NN - NX + j] = x0[(size_t)b * NX + j];
        bs.parameters(b)[0] = 2.0;
    }
}

static void RegisteredBatchRefinesAfterEnableRefine() {
    std::printf("RegisteredBatchRefinesAfterEnableRefine\n");
    const int B = 9;
    const std::vector<double> x0 = states(B);
    std::vector<double> u((size_t)B * NU), gain_b, gain_u, after_b, after_u, before_u;
    BatchMPC<RobotOCP> builtin(B);
    setup(builtin, B);
    EXPECT_EQ(builtin.enable_refine(), PMPC_ERR_INVALID_ARGUMENT);   // a built-in OCP has its lineariser in the library
    EXPECT_EQ(builtin.step(x0.data(), u.data()), PMPC_OK);
    EXPECT_EQ(builtin.refine(gain_b), PMPC_OK);
    EXPECT_EQ(builtin.solution(after_b), PMPC_OK);

    BatchMPC<UserRobotOCP> user(B);
    setup(user, B);
    EXPECT_EQ(user.step(x0.data(), u.data()), PMPC_OK);
    EXPECT_EQ(user.solution(before_u), PMPC_OK);
    EXPECT_EQ(user.refine(gain_u), PMPC_ERR_UNKNOWN_MODEL);          // nothing installs the lineariser implicitly
    EXPECT_EQ(user.enable_refine(), PMPC_OK);
    EXPECT_EQ(user.refine(gain_u, 9), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_EQ(user.refine(gain_u), PMPC_OK);
    EXPECT_EQ(user.solution(after_u), PMPC_OK);
    EXPECT_TRUE(same(gain_u, gain_b) && same(after_u, after_b) && !same(after_u, before_u));
    int accepted = 0;
    for (int b = 0; b < B; ++b) {
        EXPECT_TRUE(std::memcmp(&user.refine_info(b), &builtin.refine_info(b), sizeof(pmpc_refine_info)) == 0);
        accepted += (user.refine_info(b).flags & PMPC_REFINE_REJECTED) == 0;
    }
    EXPECT_TRUE(accepted >= B / 2);
    std::printf("  %d of %d accepted, du0/dx0 of instance 0 = %.4f\n", accepted, B, gain_u[0]);

    // enable_refine() before the first step is remembered until the batch exists
    BatchMPC<UserRobotOCP> early(B);
    setup(early, B);
    std::vector<double> gain_e, after_e;
    EXPECT_EQ(early.enable_refine(), PMPC_OK);
    EXPECT_EQ(early.step(x0.data(), u.data()), PMPC_OK);
    EXPECT_EQ(early.refine(gain_e), PMPC_OK);
    EXPECT_EQ(early.solution(after_e), PMPC_OK);
    EXPECT_TRUE(same(gain_e, gain_b) && same(after_e, after_b));
}

static void RegisteredSolversRefine() {
    std::printf("RegisteredSolversRefine\n");
    const int B = 9;
    const std::vector<double> x0 = states(B);
    const std::vector<int> sens = {NX * NN - 3, NX * NN - 2, NX * NN - 1};
    BatchSolver<RobotOCP> bb(B);
    BatchSolver<UserRobotOCP> bu(B);
    setup_solver(bb, B, x0); setup_solver(bu, B, x0);
    std::vector<double> dz_b, dz_u;
    EXPECT_EQ(bb.solve(), PMPC_OK);
    EXPECT_EQ(bu.solve(), PMPC_OK);
    for (int b = 0; b < B; ++b) EXPECT_TRUE(std::memcmp(bu.primal_solution(b), bb.primal_solution(b), N * sizeof(double)) == 0);
    EXPECT_EQ(bb.refine(3, -1.0, sens, &dz_b), PMPC_OK);
    EXPECT_EQ(bu.refine(3, -1.0, sens), PMPC_ERR_INVALID_ARGUMENT);   // sensitivities without a place for them
    EXPECT_EQ(bu.refine(3, -1.0, sens, &dz_u), PMPC_OK);
    EXPECT_TRUE(same(dz_u, dz_b));
    bool any_dz = false;
    for (double v : dz_u) any_dz = any_dz || v != 0.0;
    EXPECT_TRUE(any_dz);
    for (int b = 0; b < B; ++b) {
        EXPECT_TRUE(std::memcmp(&bu.refine_info(b), &bb.refine_info(b), sizeof(pmpc_refine_info)) == 0);
        EXPECT_TRUE(std::memcmp(bu.primal_solution(b), bb.primal_solution(b), N * sizeof(double)) == 0);
        EXPECT_TRUE(std::memcmp(bu.dual_solution(b), bb.dual_solution(b), (N + NX * NN) * sizeof(double)) == 0);
    }

    Solver<RobotOCP> sb;
    Solver<UserRobotOCP> su;
    sb.get_problem().set_time_limits(0, 2); su.get_problem().set_time_limits(0, 2);
    for (int i = 0; i < N; ++i) {
        sb.lower_bound_x()(i) = su.lower_bound_x()(i) = bb.lower_bound_x(0)[i];
        sb.upper_bound_x()(i) = su.upper_bound_x()(i) = bb.upper_bound_x(0)[i];
    }
    sb.parameters()(0) = 2.0; su.parameters()(0) = 2.0;
    sb.solve(); su.solve();
    const bool ok_b = sb.refine(), ok_u = su.refine();
    EXPECT_EQ(ok_u, ok_b);
    EXPECT_EQ(ok_u, (bu.refine_info(0).flags & PMPC_REFINE_REJECTED) == 0);
    EXPECT_TRUE(std::memcmp(&su.refine_info(), &sb.refine_info(), sizeof(pmpc_refine_info)) == 0);
    EXPECT_TRUE(std::memcmp(su.primal_solution().data(), sb.primal_solution().data(), N * sizeof(double)) == 0);
    EXPECT_TRUE(std::memcmp(su.primal_solution().data(), bu.primal_solution(0), N * sizeof(double)) == 0);
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    RegisteredBatchRefinesAfterEnableRefine();
    RegisteredSolversRefine();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
