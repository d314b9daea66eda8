// BatchMPC<OCP>::refine, BatchSolver<OCP>::refine and Solver<OCP>::refine (pmpc_mpc_batch_refine, pmpc_sqp_refine_batch): the three agree bit for bit
// on the same problems, accepted instances end with a smaller KKT residual, the gain is the rows of dz at the last node of the u block, and a
// registered OCP's batch is refused. Without a GPU the binary exits 77 (there is no CPU fallback).
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

static void RefineOnTheBatchAndOnTheSolvers() {
    std::printf("RefineOnTheBatchAndOnTheSolvers\n");
    const int B = 9;
    const std::vector<double> x0 = states(B);
    BatchMPC<RobotOCP> mpc(B);
    setup(mpc, B);
    std::vector<double> gain, u((size_t)B * NU), before, after;
    EXPECT_EQ(mpc.refine(gain), PMPC_ERR_INVALID_ARGUMENT);   // nothing resident before the first step
    EXPECT_EQ(mpc.step(x0.data(), u.data()), PMPC_OK);
    EXPECT_EQ(mpc.solution(before), PMPC_OK);
    EXPECT_EQ(mpc.refine(gain, 9), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_EQ(mpc.refine(gain), PMPC_OK);
    EXPECT_EQ(mpc.solution(after), PMPC_OK);
    EXPECT_EQ(gain.size(), (size_t)B * NU * NX);

    // the same problems through BatchSolver: solve, then refine with the sensitivities of the pinned state
    BatchSolver<RobotOCP> bs(B);
    bs.get_problem().set_time_limits(0, 2);
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < NN; ++k) { bs.lower_bound_x(b)[NX * NN + NU * k] = -0.6; bs.upper_bound_x(b)[NX * NN + NU * k] = 0.6;
                                       bs.lower_bound_x(b)[NX * NN + NU * k + 1] = -0.3; bs.upper_bound_x(b)[NX * NN + NU * k + 1] = 0.3; }
        for (int j = 0; j < NX; ++j) bs.lower_bound_x(b)[NX * NN - NX + j] = bs.upper_bound_x(b)[NX * NN - NX + j] = x0[(size_t)b * NX + j];
        bs.parameters(b)[0] = 2.0;
    }
    EXPECT_EQ(bs.solve(), PMPC_OK);
    for (int b = 0; b < B; ++b) EXPECT_TRUE(std::memcmp(bs.primal_solution(b), &before[(size_t)b * N], N * sizeof(double)) == 0);
    std::vector<double> dz;
    const std::vector<int> sens = {NX * NN - 3, NX * NN - 2, NX * NN - 1};
    EXPECT_EQ(bs.refine(3, -1.0, sens), PMPC_ERR_INVALID_ARGUMENT);   // sensitivities without a place for them
    EXPECT_EQ(bs.refine(3, -1.0, sens, &dz), PMPC_OK);
    int accepted = 0;
    for (int b = 0; b < B; ++b) {
        const pmpc_refine_info &ri = bs.refine_info(b), &mi = mpc.refine_info(b);
        EXPECT_TRUE(std::memcmp(&ri, &mi, sizeof(ri)) == 0);
        EXPECT_TRUE(std::memcmp(bs.primal_solution(b), &after[(size_t)b * N], N * sizeof(double)) == 0);
        const bool rejected = (ri.flags & PMPC_REFINE_REJECTED) != 0;
        if (rejected) EXPECT_TRUE(std::memcmp(&after[(size_t)b * N], &before[(size_t)b * N], N * sizeof(double)) == 0);
        else { ++accepted; EXPECT_TRUE(ri.r_last < ri.r_0 && ri.steps == 3 && ri.active_rows == NX * NN && ri.active_vars >= NX); }
        for (int c = 0; c < NU; ++c)
            for (int j = 0; j < NX; ++j) EXPECT_EQ(gain[((size_t)b * NU + c) * NX + j], dz[((size_t)b * NX + j) * N + NX * NN + NU * (NN - 1) + c]);
        std::printf("  instance %d: r_0 %.3e -> r_last %.3e, flags %d, du0/dx0 = %.4f\n", b, ri.r_0, ri.r_last, ri.flags, gain[(size_t)b * NU * NX]);
    }
    EXPECT_TRUE(accepted >= B / 2);

    // one problem through Solver<OCP>
    Solver<RobotOCP> s;
    s.get_problem().set_time_limits(0, 2);
    for (int i = 0; i < N; ++i) { s.lower_bound_x()(i) = bs.lower_bound_x(0)[i]; s.upper_bound_x()(i) = bs.upper_bound_x(0)[i]; }
    s.parameters()(0) = 2.0;
    s.solve();
    const bool ok = s.refine();
    EXPECT_EQ(ok, (bs.refine_info(0).flags & PMPC_REFINE_REJECTED) == 0);
    EXPECT_TRUE(std::memcmp(&s.refine_info(), &bs.refine_info(0), sizeof(pmpc_refine_info)) == 0);
    EXPECT_TRUE(std::memcmp(s.primal_solution().data(), bs.primal_solution(0), N * sizeof(double)) == 0);

    // a registered OCP has no linearisation entry
    BatchMPC<UserRobotOCP> user(B);
    setup(user, B);
    EXPECT_EQ(user.step(x0.data(), u.data()), PMPC_OK);
    EXPECT_EQ(user.refine(gain), PMPC_ERR_UNKNOWN_MODEL);
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    RefineOnTheBatchAndOnTheSolvers();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
