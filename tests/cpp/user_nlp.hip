// USER-defined NLPs compiled for the GPU in the user's own translation unit (what a PolyMPC user does with their ProblemBase subclass).
// UserHS071 restates HS071 of tests/solvers/sqp/sqp_test_autodiff.cpp:191-221 from the "user" side, so the tests can check that the
// registration path gives bit-identical results to the built-in problem; ParamHS071 is the same problem with its constant 40 as the
// static parameter p(0) (NP = 1); Wide65 has 60 variables and 5 equalities — 65 KKT rows, one more than this route serves.
#include <polympc/register_nlp.hpp>

struct UserHS071 {
    enum { NX = 4, NE = 1, NI = 1, NP = 0 };
    template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double>, T& cost) const { cost = x(0) * x(3) * (x(0) + x(1) + x(2)) + x(2); }
    template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double>, pmpc::vref<T> ce) const {
        ce(0) = (x(0) * x(0) + x(1) * x(1) + x(2) * x(2) + x(3) * x(3)) - T(40.0);
    }
    template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double>, pmpc::vref<T> ci) const { ci(0) = x(0) * x(1) * x(2) * x(3); }
};
PMPC_REGISTER_NLP(UserHS071)

struct ParamHS071 {
    enum { NX = 4, NE = 1, NI = 1, NP = 1 };
    template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double>, T& cost) const { cost = x(0) * x(3) * (x(0) + x(1) + x(2)) + x(2); }
    template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ce) const {
        ce(0) = (x(0) * x(0) + x(1) * x(1) + x(2) * x(2) + x(3) * x(3)) - T(p(0));
    }
    template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double>, pmpc::vref<T> ci) const { ci(0) = x(0) * x(1) * x(2) * x(3); }
};
PMPC_REGISTER_NLP(ParamHS071)

struct Wide65 {
    enum { NX = 60, NE = 5, NI = 0, NP = 0 };
    template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double>, T& cost) const {
        T c(0.0);
        for (int i = 0; i < NX; ++i) c = c + x(i) * x(i);
        cost = c;
    }
    template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double>, pmpc::vref<T> ce) const {
        for (int k = 0; k < NE; ++k) ce(k) = x(k) - T(1.0);
    }
    template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T>, pmpc::cref<double>, pmpc::vref<T>) const {}
};
PMPC_REGISTER_NLP(Wide65)
