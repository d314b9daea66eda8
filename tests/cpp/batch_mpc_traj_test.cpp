// BatchMPC<OCP>::solution_x_at(t) / solution_u_at(t) / shift(dt) (pmpc_mpc_batch_sample / _shift: the interpolant evaluated on the device)
// against MPC<OCP>::solution_x_at(t) / solution_u_at(t) of the host mirror holding the same iterate. The host compiler may contract a * b + c,
// so the comparison is not bit for bit: each weight takes at most 3P + 1 roundings and the sum P + 1; doubled,
//   |device - host| <= 8 (P + 1) eps sum_i |l_i| |v_i|.
// Without a GPU the binary exits 77 (there is no CPU fallback).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include <polympc/polympc.hpp>

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("  EXPECT_TRUE failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++failures; } } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

using namespace polympc;

// sum_i |l_i| |v_i| of one component at time t: the basis as MPC<OCP>::interpolate builds it
template <class mpc_t>
static double bound_scale(const mpc_t& one, double t0, double tf, double t, bool control, int c) {
    constexpr int P = mpc_t::npn - 1, S = mpc_t::num_segms, nn = mpc_t::num_nodes;
    mpc_t& m = const_cast<mpc_t&>(one);
    const double L = (tf - t0) / S;
    const int idx = std::max(0, std::min((int)std::floor(t / L), S - 1));
    const double tl = t - idx * L;
    double s[P + 1];
    for (int j = 0; j <= P; ++j) s[j] = m.ocp().time_nodes(nn - 1 - j);
    double sum = 0.0;
    for (int i = 0; i <= P; ++i) {
        double li = 1.0;
        for (int j = 0; j <= P; ++j) if (j != i) li *= (tl - s[j]) / (s[i] - s[j]);
        const double v = control ? one.solution_u_at(idx * P + i)(c) : one.solution_x_at(idx * P + i)(c);
        sum += std::fabs(li) * std::fabs(v);
    }
    return sum;
}

template <int P, int S>
static void BatchMPCTrajectoryTest() {
    std::printf("BatchMPCTrajectoryTest<%d, %d>\n", P, S);
    using OCP = polympc::models::MobileRobot<polympc::Spline<polympc::Chebyshev<P, polympc::GAUSS_LOBATTO, double>, S>>;
    using mpc_t = MPC<OCP>;
    constexpr int nx = mpc_t::nx, nu = mpc_t::nu, nn = mpc_t::num_nodes, var = mpc_t::var_size;
    const double tf = 2.0, eps = std::numeric_limits<double>::epsilon(), tol = 8.0 * (P + 1) * eps;
    const int B = 5;
    BatchMPC<OCP> mpc(B);
    std::vector<double> out;
    EXPECT_EQ(mpc.solution_x_at(0.5, out), PMPC_ERR_INVALID_ARGUMENT);   // nothing resident before the first step
    EXPECT_EQ(mpc.shift(0.1), PMPC_ERR_INVALID_ARGUMENT);
    mpc.ocp().set_Q_coeff(2.0);
    mpc.settings().max_iter = 10; mpc.settings().line_search_max_iter = 10;
    mpc.set_time_limits(0, tf);
    Vector<2> lbu, ubu; lbu(0) = -1.5; lbu(1) = -0.75; ubu(0) = 1.5; ubu(1) = 0.75;
    Vector<1> p; p(0) = 2.0;
    for (int b = 0; b < B; ++b) { mpc.control_bounds(b, lbu, ubu); mpc.set_static_parameters(b, p); }
    std::vector<double> x0(B * nx), u0(B * nu);
    for (int b = 0; b < B; ++b) { x0[nx * b] = 0.5 + 0.05 * b; x0[nx * b + 1] = 0.5 - 0.03 * b; x0[nx * b + 2] = 0.5; }
    EXPECT_EQ(mpc.step(x0.data(), u0.data()), PMPC_OK);

    std::vector<double> iter;
    EXPECT_EQ(mpc.solution(iter), PMPC_OK);
    std::vector<mpc_t> host(B);
    for (int b = 0; b < B; ++b) {
        host[b].set_time_limits(0, tf);
        typename mpc_t::traj_state_t xg; typename mpc_t::traj_control_t ug;
        for (int i = 0; i < nx * nn; ++i) xg(i) = iter[(size_t)b * var + i];
        for (int i = 0; i < nu * nn; ++i) ug(i) = iter[(size_t)b * var + nx * nn + i];
        host[b].x_guess(xg); host[b].u_guess(ug);
    }
    std::vector<double> times;
    for (int k = 0; k < nn; ++k) times.push_back(host[0].ocp().time_nodes(nn - 1 - k));
    for (int k = 0; k <= S; ++k) times.push_back(k * (tf / S));
    for (int q = 0; q <= 20; ++q) times.push_back(tf * q / 20.0 + 0.013);
    times.push_back(-0.1); times.push_back(tf + 0.1);
    std::vector<double> xs, us;
    for (double t : times) {
        EXPECT_EQ(mpc.solution_x_at(t, xs), PMPC_OK);
        EXPECT_EQ(mpc.solution_u_at(t, us), PMPC_OK);
        EXPECT_EQ(xs.size(), (size_t)B * nx); EXPECT_EQ(us.size(), (size_t)B * nu);
        for (int b = 0; b < B; ++b) {
            const auto hx = host[b].solution_x_at(t); const auto hu = host[b].solution_u_at(t);
            for (int c = 0; c < nx; ++c) EXPECT_TRUE(std::fabs(xs[b * nx + c] - hx(c)) <= tol * bound_scale(host[b], 0, tf, t, false, c));
            for (int c = 0; c < nu; ++c) EXPECT_TRUE(std::fabs(us[b * nu + c] - hu(c)) <= tol * bound_scale(host[b], 0, tf, t, true, c));
        }
    }
    // u(t_start) of the step is the interpolant at 0 on one segment (the node value itself)
    EXPECT_EQ(mpc.solution_u_at(0.0, us), PMPC_OK);
    if (S == 1) for (int i = 0; i < B * nu; ++i) EXPECT_EQ(us[i], u0[i]);

    // shift(dt): forward node k receives the old interpolant at min(t_k + dt, tf); the next step starts from it
    const double dt = 0.1;
    EXPECT_EQ(mpc.shift(-1.0), PMPC_ERR_INVALID_ARGUMENT);
    EXPECT_EQ(mpc.shift(dt), PMPC_OK);
    std::vector<double> moved;
    EXPECT_EQ(mpc.solution(moved), PMPC_OK);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nn; ++k) {
            const double t = std::min(host[b].ocp().time_nodes(nn - 1 - k) + dt, tf);
            const auto hx = host[b].solution_x_at(t); const auto hu = host[b].solution_u_at(t);
            for (int c = 0; c < nx; ++c)
                EXPECT_TRUE(std::fabs(moved[(size_t)b * var + (nn - 1 - k) * nx + c] - hx(c)) <= tol * bound_scale(host[b], 0, tf, t, false, c));
            for (int c = 0; c < nu; ++c)
                EXPECT_TRUE(std::fabs(moved[(size_t)b * var + nx * nn + (nn - 1 - k) * nu + c] - hu(c)) <= tol * bound_scale(host[b], 0, tf, t, true, c));
        }
    EXPECT_EQ(mpc.shift(dt, true), PMPC_OK);
    EXPECT_EQ(mpc.step(x0.data(), u0.data()), PMPC_OK);
    for (int b = 0; b < B; ++b) EXPECT_TRUE(mpc.info(b).status == (int)PMPC_SQP_SOLVED || mpc.info(b).status == (int)PMPC_SQP_MAX_ITER_EXCEEDED);
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    BatchMPCTrajectoryTest<6, 1>();
    BatchMPCTrajectoryTest<5, 3>();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
