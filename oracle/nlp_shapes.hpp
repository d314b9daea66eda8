// ORACLE — TEST INFRASTRUCTURE ONLY.
//
// Generic NLPs that span the size range of the device NLP route (pmpc_nlp.hpp: up to 64 KKT rows), written ONCE and compiled by both
// sides: hipcc builds them into tests/cpp/user_nlp_shapes.hip (pmpc::Dual, cref / vref views) and g++ into the checker (oracle::Dual,
// pointer views, oracle/nlp.hpp ShapeDef). The bodies use + - * / only, with every constant written as T(c), so both AD layers run the
// same operations in the same order.
//
// A body is   enum { NX, NE, NI, NP };   cost<T>(x, p, c);   eq<T>(x, p, ce);   ineq<T>(x, p, ci);
// where x(i), p(i) read and ce(i) / ci(i) write. Most problems are MANUFACTURED: a target point xs, multipliers for some of the
// constraints and bounds (lower-active < 0, upper-active > 0, the rest 0) and a strictly convex cost term sum_i w_i (x_i - a_i)^2 whose
// data a is chosen so that stationarity holds at xs: a_i = xs_i + (J' lam + lam_box)_i / (2 w_i). The coupling terms are built from
// d = x - xs, so their gradient vanishes at xs while their Hessian does not. The tests recompute xs, the multipliers, the bounds and every
// derivative in numpy (tests/test_gpu_nlp_shapes.py) and keep the indices and constants below in step with it.
#pragma once

#if defined(__HIPCC__)
#define NLP_SHAPE_FN __host__ __device__ static
#else
#define NLP_SHAPE_FN static
#endif

namespace nlp_shapes {

// chained Rosenbrock, 9 variables: x* = 1. Odd NX (the round-robin Jacobi's dummy pair), two Hessian passes of 64 entries.
struct ChainRosen9 {
    enum { NX = 9, NE = 0, NI = 0, NP = 0 };
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P&, T& c) {
        T s(0.0);
        for (int i = 0; i + 1 < NX; ++i) {
            const T r = x(i + 1) - x(i) * x(i), o = T(1.0) - x(i);
            s = s + T(100.0) * r * r + o * o;
        }
        c = s;
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X&, const P&, O&) {}
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X&, const P&, O&) {}
};

// the cost shared by the manufactured shapes: sum w_i (x_i - a_i)^2 + kappa sum d_i d_{i+1} + gamma sum d_i^2 d_{i+1}, d = x - xs
template <class T, class X, class S> NLP_SHAPE_FN T coupled_cost(const X& x, int n, double kappa, double gamma) {
    T s(0.0);
    for (int i = 0; i < n; ++i) { const T e = x(i) - T(S::a(i)); s = s + T(S::w(i)) * e * e; }
    for (int i = 0; i + 1 < n; ++i) {
        const T di = x(i) - T(S::xs(i)), dj = x(i + 1) - T(S::xs(i + 1));
        s = s + T(kappa) * di * dj + T(gamma) * di * di * dj;
    }
    return s;
}
NLP_SHAPE_FN double weight(int i) { return 1.0 + 0.25 * (i % 4); }

// projection on a sphere with a coupled cost, 12 variables, 1 equality sum x_i^2 = R^2 (multiplier 0.5)
struct Sphere12 {
    enum { NX = 12, NE = 1, NI = 0, NP = 0 };
    NLP_SHAPE_FN double xs(int i) { return 0.2 + 0.05 * i; }
    NLP_SHAPE_FN double w(int i) { return weight(i); }
    NLP_SHAPE_FN double a(int i) { return xs(i) + 0.5 * xs(i) / w(i); }
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P&, T& c) { c = coupled_cost<T, X, Sphere12>(x, NX, 0.3, 0.5); }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X& x, const P&, O& ce) {
        T s(0.0);
        double r2 = 0.0;
        for (int i = 0; i < NX; ++i) { s = s + x(i) * x(i); r2 += xs(i) * xs(i); }
        ce(0) = s - T(r2);
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X&, const P&, O&) {}
};

// 8 variables, 40 inequalities g_k = sum_j C_kj x_j + beta_k x_{k%8}^2; g_0, g_1 active at their lower bound, g_2, g_3 at their upper bound,
// x_1 at its lower bound, x_6 at its upper bound, everything else inactive
struct Cuts8 {
    enum { NX = 8, NE = 0, NI = 40, NP = 0 };
    NLP_SHAPE_FN double xs(int i) { return 0.5 + 0.1 * i; }
    NLP_SHAPE_FN double w(int i) { return weight(i); }
    NLP_SHAPE_FN double C(int k, int j) { return ((3 * k + 5 * j) % 7 - 3) * 0.25; }
    NLP_SHAPE_FN double beta(int k) { return 0.1 * (k % 3); }
    NLP_SHAPE_FN double lam_g(int k) { return k == 0 ? -0.5 : k == 1 ? -0.3 : k == 2 ? 0.4 : k == 3 ? 0.7 : 0.0; }
    NLP_SHAPE_FN double lam_x(int i) { return i == 1 ? -0.6 : i == 6 ? 0.4 : 0.0; }
    NLP_SHAPE_FN double a(int i) {
        double g = 0.0;
        for (int k = 0; k < NI; ++k) g += lam_g(k) * (C(k, i) + (k % NX == i ? 2.0 * beta(k) * xs(i) : 0.0));
        return xs(i) + (g + lam_x(i)) / (2.0 * w(i));
    }
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P&, T& c) { c = coupled_cost<T, X, Cuts8>(x, NX, 0.3, 0.5); }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X&, const P&, O&) {}
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X& x, const P&, O& ci) {
        for (int k = 0; k < NI; ++k) {
            T s(0.0);
            for (int j = 0; j < NX; ++j) s = s + T(C(k, j)) * x(j);
            ci(k) = s + T(beta(k)) * x(k % NX) * x(k % NX);
        }
    }
};

// 32 variables, 16 bilinear equalities x_k x_{16+k} = xs_k xs_{16+k}, 16 inequalities x_k^2 + x_{16+k}^2 + p1 d_{(k+5)%32}^2 (g_0, g_1
// lower-active, g_2, g_3 upper-active), x_8 at its lower bound, x_25 at its upper bound: 64 KKT rows. p0 scales the cost's coupling.
struct Wave64 {
    enum { NX = 32, NE = 16, NI = 16, NP = 2 };
    NLP_SHAPE_FN double xs(int i) { return i < 16 ? 0.6 + 0.03 * i : 1.1 + 0.02 * (i - 16); }
    NLP_SHAPE_FN double w(int i) { return weight(i); }
    NLP_SHAPE_FN double lam_e(int k) { return 0.3 - 0.04 * k; }
    NLP_SHAPE_FN double lam_g(int k) { return k == 0 ? -0.2 : k == 1 ? -0.15 : k == 2 ? 0.5 : k == 3 ? 0.3 : 0.0; }
    NLP_SHAPE_FN double lam_x(int i) { return i == 8 ? -0.5 : i == 25 ? 0.35 : 0.0; }
    NLP_SHAPE_FN double a(int i) {
        const int k = i % 16, o = i < 16 ? i + 16 : i - 16;
        const double g = lam_e(k) * xs(o) + lam_g(k) * 2.0 * xs(i);
        return xs(i) + (g + lam_x(i)) / (2.0 * w(i));
    }
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P& p, T& c) {
        T s(0.0);
        for (int i = 0; i < NX; ++i) { const T e = x(i) - T(a(i)); s = s + T(w(i)) * e * e; }
        const T kap = T(0.2) * T(p(0));
        for (int i = 0; i + 1 < NX; ++i) s = s + kap * (x(i) - T(xs(i))) * (x(i + 1) - T(xs(i + 1)));
        c = s;
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X& x, const P&, O& ce) {
        for (int k = 0; k < NE; ++k) ce(k) = x(k) * x(16 + k) - T(xs(k) * xs(16 + k));
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X& x, const P& p, O& ci) {
        for (int k = 0; k < NI; ++k) {
            const int r = (k + 5) % NX;
            const T dr = x(r) - T(xs(r));
            ci(k) = x(k) * x(k) + x(16 + k) * x(16 + k) + T(p(1)) * dr * dr;
        }
    }
};

// 60 variables (the largest NX beside 4 equalities), 4 equalities sum_{j = k mod 4} x_j^2 = sum xs_j^2, x_10 at its lower bound, x_33 at
// its upper bound
struct Wide60 {
    enum { NX = 60, NE = 4, NI = 0, NP = 0 };
    NLP_SHAPE_FN double xs(int i) { return 0.3 + 0.01 * i; }
    NLP_SHAPE_FN double w(int i) { return weight(i); }
    NLP_SHAPE_FN double lam_e(int k) { return k == 0 ? 0.4 : k == 1 ? -0.3 : k == 2 ? 0.2 : -0.1; }
    NLP_SHAPE_FN double lam_x(int i) { return i == 10 ? -0.5 : i == 33 ? 0.3 : 0.0; }
    NLP_SHAPE_FN double a(int i) { return xs(i) + (lam_e(i % 4) * 2.0 * xs(i) + lam_x(i)) / (2.0 * w(i)); }
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P&, T& c) { c = coupled_cost<T, X, Wide60>(x, NX, 0.3, 0.5); }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X& x, const P&, O& ce) {
        for (int k = 0; k < NE; ++k) {
            T s(0.0);
            double r2 = 0.0;
            for (int j = k; j < NX; j += NE) { s = s + x(j) * x(j); r2 += xs(j) * xs(j); }
            ce(k) = s - T(r2);
        }
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X&, const P&, O&) {}
};

// 64 variables, no constraints: x* = xs (the coupled cost's minimiser: a = xs)
struct Unc64 {
    enum { NX = 64, NE = 0, NI = 0, NP = 0 };
    NLP_SHAPE_FN double xs(int i) { return 0.5 + 0.01 * i; }
    NLP_SHAPE_FN double w(int i) { return weight(i); }
    NLP_SHAPE_FN double a(int i) { return xs(i); }
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P&, T& c) { c = coupled_cost<T, X, Unc64>(x, NX, 0.3, 0.5); }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X&, const P&, O&) {}
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X&, const P&, O&) {}
};

// 10 variables, 2 equalities, 3 inequalities, 70 static parameters; every datum is a parameter (the tests manufacture them per instance):
//   cost = sum_i p[10+i] (x_i - p[i])^2 + sum_{i<9} p[20+i] x_i x_{i+1} + p[69] x_0 x_9
//   h_0 = sum_j p[30+j] x_j^2 - p[60],   h_1 = sum_j p[40+j] x_j - p[61]
//   g_k = p[50+k] x_k^2 + p[64+k] x_{k+3} x_{k+4} + p[67+k] x_{k+6}   (k = 0, 1, 2)
struct Param70 {
    enum { NX = 10, NE = 2, NI = 3, NP = 70 };
    template <class T, class X, class P> NLP_SHAPE_FN void cost(const X& x, const P& p, T& c) {
        T s(0.0);
        for (int i = 0; i < NX; ++i) { const T e = x(i) - T(p(i)); s = s + T(p(10 + i)) * e * e; }
        for (int i = 0; i + 1 < NX; ++i) s = s + T(p(20 + i)) * x(i) * x(i + 1);
        c = s + T(p(69)) * x(0) * x(9);
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void eq(const X& x, const P& p, O& ce) {
        T s(0.0), l(0.0);
        for (int j = 0; j < NX; ++j) { s = s + T(p(30 + j)) * x(j) * x(j); l = l + T(p(40 + j)) * x(j); }
        ce(0) = s - T(p(60));
        ce(1) = l - T(p(61));
    }
    template <class T, class X, class P, class O> NLP_SHAPE_FN void ineq(const X& x, const P& p, O& ci) {
        for (int k = 0; k < NI; ++k) ci(k) = T(p(50 + k)) * x(k) * x(k) + T(p(64 + k)) * x(k + 3) * x(k + 4) + T(p(67 + k)) * x(k + 6);
    }
};

}  // namespace nlp_shapes
