// Host-side NLP tests written like the reference's own gtest cases (tests/solvers/sqp/sqp_test_autodiff.cpp), against the generic-NLP
// surface of include/polympc/polympc.hpp:
//   TestConstrainedRosenbrock / TestRosenbrock / TestSimpleNLP / TestHS071   sqp_test_autodiff.cpp:78-97, :119-137, :165-186, :223-246
//                                                                              (built-in device code, POLYMPC_USE_BUILTIN_NLP)
//   the same HS071 through a user-registered problem (user_nlp.hip, POLYMPC_USE_REGISTERED_NLP) and as a batch (NlpBatchSolver)
// The reference's SQPSolver installs eigenvalue mirroring as its Hessian regularisation: settings().regularisation = 1 here.
// HS071's `iter < max_iter` is not asserted: the iteration count of that problem is decided by rounding (tests/test_oracle_pins.py,
// test_sqp_hs071_iteration_bound_is_a_last_bit_property); the solution is.
#include <cstdio>
#include <limits>
#include <polympc/polympc.hpp>

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("  EXPECT_TRUE failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++failures; } } while (0)
#define EXPECT_LT(a, b) EXPECT_TRUE((a) < (b))
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

using namespace polympc;

POLYMPC_FORWARD_NLP_DECLARATION(/*Name*/ ConstrainedRosenbrock, /*NX*/ 2, /*NE*/ 1, /*NI*/ 0, /*NP*/ 0, /*Type*/ double)
class ConstrainedRosenbrock : public ProblemBase<ConstrainedRosenbrock> {
public:
    nlp_variable_t SOLUTION = make(0.7864, 0.6177);
    static nlp_variable_t make(double a, double b) { nlp_variable_t v; v(0) = a; v(1) = b; return v; }
};
POLYMPC_USE_BUILTIN_NLP(ConstrainedRosenbrock, PMPC_NLP_CONSTRAINED_ROSENBROCK)

POLYMPC_FORWARD_NLP_DECLARATION(Rosenbrock, 2, 0, 0, 0, double)
class Rosenbrock : public ProblemBase<Rosenbrock> {
public:
    nlp_variable_t SOLUTION = nlp_variable_t::Constant(1.0);
};
POLYMPC_USE_BUILTIN_NLP(Rosenbrock, PMPC_NLP_ROSENBROCK)

POLYMPC_FORWARD_NLP_DECLARATION(SimpleNLP, 2, 0, 1, 0, double)
class SimpleNLP : public ProblemBase<SimpleNLP> {
public:
    nlp_variable_t SOLUTION = nlp_variable_t::Constant(1.0);
};
POLYMPC_USE_BUILTIN_NLP(SimpleNLP, PMPC_NLP_SIMPLE)

static Vector<4> hs071_solution() { Vector<4> s; s(0) = 1.00000000; s(1) = 4.74299963; s(2) = 3.82114998; s(3) = 1.37940829; return s; }
POLYMPC_FORWARD_NLP_DECLARATION(HS071, 4, 1, 1, 0, double)
class HS071 : public ProblemBase<HS071> {
public:
    nlp_variable_t SOLUTION = hs071_solution();
};
POLYMPC_USE_BUILTIN_NLP(HS071, PMPC_NLP_HS071)

// the same problem with its device code from the user's library (user_nlp.hip)
struct UserHS071 {};
POLYMPC_FORWARD_NLP_DECLARATION(UserHS071Problem, 4, 1, 1, 0, double)
class UserHS071Problem : public ProblemBase<UserHS071Problem> {
public:
    nlp_variable_t SOLUTION = hs071_solution();
    UserHS071 device_problem() const { return UserHS071(); }
};
POLYMPC_USE_REGISTERED_NLP(UserHS071Problem, UserHS071)

template <class Problem>
static void two_variable_case(const char* name, double x00, double x01, bool ring) {
    std::printf("%s\n", name);
    using Solver = NlpSolver<Problem>;
    Problem problem;
    Solver solver;
    typename Solver::nlp_variable_t x0, x;
    typename Solver::nlp_dual_t y0;
    y0.setZero();
    x0(0) = x00; x0(1) = x01;
    solver.settings().max_iter = 50;
    solver.settings().line_search_max_iter = 5;
    solver.settings().regularisation = 1;
    if (ring) { solver.lower_bound_g()(0) = 1; solver.upper_bound_g()(0) = 2; }
    solver.solve(x0, y0);
    x = solver.primal_solution();
    EXPECT_TRUE(x.isApprox(problem.SOLUTION, 1e-2));
    EXPECT_LT(solver.info().iter, solver.settings().max_iter);
    EXPECT_EQ(last_error(), PMPC_OK);
}

template <class Problem>
static void hs071_case(const char* name, typename NlpSolver<Problem>::nlp_variable_t* out) {
    std::printf("%s\n", name);
    using Solver = NlpSolver<Problem>;
    Problem problem;
    Solver solver;
    typename Solver::nlp_variable_t x0, x;
    typename Solver::nlp_dual_t y0;
    y0.setZero();
    x0(0) = 1.0; x0(1) = 5.0; x0(2) = 5.0; x0(3) = 1.0;
    solver.settings().max_iter = 50;
    solver.settings().line_search_max_iter = 5;
    solver.settings().regularisation = 1;
    solver.lower_bound_x() = Solver::nlp_variable_t::Constant(1.0);
    solver.upper_bound_x() = Solver::nlp_variable_t::Constant(5.0);
    solver.lower_bound_g()(0) = 25;
    solver.upper_bound_g()(0) = std::numeric_limits<double>::infinity();
    solver.solve(x0, y0);
    x = solver.primal_solution();
    EXPECT_TRUE(x.isApprox(problem.SOLUTION, 1e-2));
    EXPECT_EQ(last_error(), PMPC_OK);
    EXPECT_TRUE(solver.primal_norm() >= 0 && solver.constr_violation() < 1e-2);
    *out = x;
}

static void HS071Batch(const Vector<4>& single) {   // 8 copies of the known-answer case, solved by one launch: each equals the single solve
    std::printf("HS071Batch\n");
    NlpBatchSolver<HS071> batch(8);
    batch.settings().max_iter = 50; batch.settings().line_search_max_iter = 5; batch.settings().regularisation = 1;
    for (int b = 0; b < 8; ++b) {
        const double x0[4] = {1.0, 5.0, 5.0, 1.0};
        for (int i = 0; i < 4; ++i) { batch.primal_solution(b)[i] = x0[i]; batch.lower_bound_x(b)[i] = 1.0; batch.upper_bound_x(b)[i] = 5.0; }
        batch.lower_bound_g(b)[0] = 25; batch.upper_bound_g(b)[0] = std::numeric_limits<double>::infinity();
    }
    EXPECT_EQ(batch.solve(), PMPC_OK);
    for (int b = 0; b < 8; ++b) for (int i = 0; i < 4; ++i) EXPECT_TRUE(batch.primal_solution(b)[i] == single(i));
}

int main() {
    if (!polympc::context()) { std::printf("no GPU: %s\n", pmpc_status_string(polympc::last_error())); return 77; }
    two_variable_case<ConstrainedRosenbrock>("TestConstrainedRosenbrock", 2.01, 1.01, false);
    two_variable_case<Rosenbrock>("TestRosenbrock", 2.01, 1.01, false);
    two_variable_case<SimpleNLP>("TestSimpleNLP", 1.0, 1.0, true);
    Vector<4> xb, xu;
    hs071_case<HS071>("TestHS071", &xb);
    hs071_case<UserHS071Problem>("TestHS071RegisteredByUser", &xu);
    for (int i = 0; i < 4; ++i) EXPECT_TRUE(xb(i) == xu(i));
    HS071Batch(xb);
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
