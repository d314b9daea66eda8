// polympc_amd — batched SQP for generic NLPs (the reference's ProblemBase problems, src/solvers/nlproblem.hpp) on the device.
//
// A problem type is the reference's NLP class written for hipcc, as register_ocp.hpp asks of an OCP:
//
//     struct MyNLP {
//         enum { NX = 4, NE = 1, NI = 1, NP = 0 };   // variables, equalities, inequalities, static parameters (POLYMPC_FORWARD_NLP_DECLARATION)
//         template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double> p, T& cost) const;
//         template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ce) const;
//         template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ci) const;
//     };
//
// nlp_kernel<Def> restates SQPBase::solve (sqp_base.hpp:569-696) for such a problem, one 64-lane wavefront per instance, with every
// vector and matrix of the iteration in LDS. It follows the CPU checker (its SQP<GenericNLP<Def>>) operation for operation:
//   * linearisation by forward AD (the checker's GenericNLP): the derivatives of the nested vector dual are component-wise, so lane j
//     evaluates the problem with a one-direction dual seeded on x_j (gradient entry j, Jacobian column j) and lane e = a + b NX a
//     second-order dual seeded on the two directions of Hessian entry (a, b) — the cost with outer seed b and inner seed a, the constraints
//     with outer seed a and inner seed b, as GenericNLP reads them (its Hessian of the cost is stored transposed, the constraint Hessians
//     are not); the entry then sums cost + lam_q * constraint entry in the checker's loop order;
//   * dense damped BFGS (bfgs.hpp:23-52) or the exact Hessian every iteration; regularisation 0 / 1 (eigenvalue mirroring with the checker's
//     Jacobi iteration: pair by pair cyclic for NX <= 8, round robin above) / 2 (Gershgorin shift);
//   * the QP is the register-resident box-ADMM boxadmm_solve_reg<NX, NE + NI> (pmpc_qp_reg.hpp) with the lower-triangle read of H and the
//     numeric conditioning gate — the checker's PIVOT_SWEEP as nlp_solve runs it. There is no full-form redo on this route: an instance
//     whose QP trips the gate stops with status 4 and PMPC_FLAG_ILLCOND, as the checker does;
//   * the l1-merit backtracking line search, the termination test and the pmpc_sqp_info fields of the fused OCP kernels.
// Every sequential sum is evaluated in the checker's order (by every lane on the same LDS values: the sizes are small); every element-wise
// update runs one element per lane. Control decisions go through readfirstlane, so the QP is always reached with every lane enabled.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/polympc_amd.h"
#include "pmpc_ad.hpp"
#include "pmpc_models.hpp"
#include "pmpc_qp.hpp"
#include "pmpc_qp_reg.hpp"

// context services exported by libpolympc_amd.so for the NLP route: selects the context's device, runs the poison harness when it is on,
// and returns the stream and the dynamic LDS limit
extern "C" pmpc_status pmpc_internal_nlp_services(pmpc_context* ctx, void** stream, size_t* lds_limit);

namespace pmpc {

constexpr int PMPC_NLP_ILLCOND_STOP = 4;   // sqp status of an instance whose QP tripped the conditioning gate (the checker's SQP_REDO)

template <class Def>
struct NlpLayout {
    enum { NX = Def::NX, NE = Def::NE, NI = Def::NI, NP = Def::NP, M = NE + NI, N = NX + M };
    enum { ML = M > 0 ? M : 1, NIL = NI > 0 ? NI : 1, NPL = NP > 0 ? NP : 1 };
    static_assert(NX > 0 && NE >= 0 && NI >= 0 && NP >= 0, "NLP dimensions");
    static constexpr bool FITS = N <= WAVE;   // one KKT row per lane
    static constexpr int tri() { if constexpr (FITS) return RegKkt<N>::TRI; else return 0; }
    // doubles, in carve order (the QP staging first: it keeps the alignment of the dynamic LDS block)
    static constexpr int TR = 0, X = TR + tri(), LAM = X + NX, LAMK = LAM + M + NX, H_ = LAMK + M + NX, LG = H_ + NX, LGN = LG + NX,
                         HH = LGN + NX, A = HH + NX * NX, AL = A + ML * NX, AU = AL + ML, LX = AU + ML, UX = LX + NX, LBX = UX + NX,
                         UBX = LBX + NX, LBG = UBX + NX, UBG = LBG + NIL, STEP = UBG + NIL, XS = STEP + NX, PX = XS + NX, PY = PX + NX,
                         PAR = PY + M + NX, BS = PAR + NPL, RR = BS + NX, EW = RR + NX, CS = EW + NX, BASE = CS + NX + 1;
    static constexpr int EA = BASE, EV = EA + NX * NX, WITH_EIG = EV + NX * NX;   // regularisation 1 only
    static size_t lds_bytes(int regularisation) { return (size_t)(regularisation == 1 ? WITH_EIG : BASE) * sizeof(double); }
};

// problem evaluations at LDS points; `p` = the instance's static parameters
template <class Def>
struct NlpEval {
    using L = NlpLayout<Def>;
    using D1 = Dual<double, 1>;
    using D2 = Dual<Dual<double, 1>, 1>;
    const Def& def;
    const double* p;

    __device__ double cost(const double* xx) const {
        Value c(0.0);
        def.template cost_impl<Value>(as_cvalues(xx), cref<double>(p), c);
        return c.v;
    }
    __device__ void equalities(const double* xx, Value* ce) const {
        if constexpr (L::NE > 0) def.template equality_constraints_impl<Value>(as_cvalues(xx), cref<double>(p), vref<Value>(ce));
    }
    __device__ void inequalities(const double* xx, Value* ci) const {
        if constexpr (L::NI > 0) def.template inequality_constraints_impl<Value>(as_cvalues(xx), cref<double>(p), vref<Value>(ci));
    }

    // GenericNLP::lagrangian_gradient: h = cost gradient, g = constraint values [eq | ineq], A = Jacobian (M x NX, column-major),
    // lg = Jacobian' lam + h + lam_box (finish_lag_grad). Lane j: direction j. Returns the cost value.
    __device__ double first_order(const double* xx, const double* lam, double* h, double* g, double* A, double* lg) const {
        const int ln = lane_id();
        const int j = ln < L::NX ? ln : L::NX - 1;
        D1 xv[L::NX];
#pragma unroll
        for (int k = 0; k < L::NX; ++k) { xv[k] = D1(xx[k]); xv[k].d[0] = (k == j) ? 1.0 : 0.0; }
        D1 c(0.0);
        def.template cost_impl<D1>(cref<D1>(xv), cref<double>(p), c);
        D1 ce[L::NE > 0 ? L::NE : 1], ci[L::NI > 0 ? L::NI : 1];
        if constexpr (L::NE > 0) def.template equality_constraints_impl<D1>(cref<D1>(xv), cref<double>(p), vref<D1>(ce));
        if constexpr (L::NI > 0) def.template inequality_constraints_impl<D1>(cref<D1>(xv), cref<double>(p), vref<D1>(ci));
        if (ln < L::NX) {
            h[j] = c.d[0];
#pragma unroll
            for (int i = 0; i < L::NE; ++i) A[i + j * L::M] = ce[i].d[0];
#pragma unroll
            for (int i = 0; i < L::NI; ++i) A[(L::NE + i) + j * L::M] = ci[i].d[0];
        }
        if (ln == 0) {
#pragma unroll
            for (int i = 0; i < L::NE; ++i) g[i] = ce[i].v;
#pragma unroll
            for (int i = 0; i < L::NI; ++i) g[L::NE + i] = ci[i].v;
        }
        wsync();
        if (ln < L::NX) {
            double a = 0.0;
            for (int i = 0; i < L::M; ++i) a += A[i + j * L::M] * lam[i];
            a += h[j];
            a += lam[L::M + j];
            lg[j] = a;
        }
        wsync();
        return c.v;
    }
    // GenericNLP::lagrangian_gradient_hessian's Hessian: H(a, b) = cost entry (outer b, inner a), then + lam_q * entry (outer a, inner b)
    // of every equality, then of every inequality
    __device__ void hessian(const double* xx, const double* lam, double* H) const {
        const int ln = lane_id();
        constexpr int NN2 = L::NX * L::NX;
        for (int e0 = 0; e0 < NN2; e0 += WAVE) {
            const int e = (e0 + ln < NN2) ? e0 + ln : NN2 - 1;
            const int a = e % L::NX, b = e / L::NX;
            D2 c(0.0);
            def.template cost_impl<D2>(cref<D2>(xx, 0, a, b), cref<double>(p), c);
            double hv = c.d[0].d[0];
            if constexpr (L::NE > 0) {
                D2 ce[L::NE];
                def.template equality_constraints_impl<D2>(cref<D2>(xx, 0, b, a), cref<double>(p), vref<D2>(ce));
#pragma unroll
                for (int q = 0; q < L::NE; ++q) hv += lam[q] * ce[q].d[0].d[0];
            }
            if constexpr (L::NI > 0) {
                D2 ci[L::NI];
                def.template inequality_constraints_impl<D2>(cref<D2>(xx, 0, b, a), cref<double>(p), vref<D2>(ci));
#pragma unroll
                for (int q = 0; q < L::NI; ++q) hv += lam[q + L::NE] * ci[q].d[0].d[0];
            }
            if (e0 + ln < NN2) H[e] = hv;
        }
        wsync();
    }
};

__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

template <class Def>
struct NlpSqp {
    using L = NlpLayout<Def>;
    static constexpr int NX = L::NX, NE = L::NE, NI = L::NI, M = L::M, N = L::N;
    static constexpr double EPS = 2.220446049250313e-16;
    NlpEval<Def> ev;
    double* s;   // the instance's LDS block (NlpLayout)
    const pmpc_sqp_settings& ss;
    const pmpc_qp_settings& qs;
    double cost_log = 0.0, primal_norm = 0.0, dual_norm = 0.0, max_violation = 0.0;
    int qp_iter_total = 0, qp_flags = 0;

    __device__ double* at(int off) const { return s + off; }

    // constraints_violation_impl :423-444
    __device__ double constraints_violation(const double* xx) const {
        Value ce[L::NE > 0 ? L::NE : 1], ci[L::NIL];
        ev.equalities(xx, ce);
        ev.inequalities(xx, ci);
        const double *lbg = at(L::LBG), *ubg = at(L::UBG), *lbx = at(L::LBX), *ubx = at(L::UBX);
        double cl1 = EPS, t = 0.0;
        for (int i = 0; i < NE; ++i) t += fabs(ce[i].v);
        cl1 += t;
        t = 0.0; for (int i = 0; i < NI; ++i) t += fmax(lbg[i] - ci[i].v, 0.0); cl1 += t;
        t = 0.0; for (int i = 0; i < NI; ++i) t += fmax(ci[i].v - ubg[i], 0.0); cl1 += t;
        t = 0.0; for (int i = 0; i < NX; ++i) t += fmax(lbx[i] - xx[i], 0.0); cl1 += t;
        t = 0.0; for (int i = 0; i < NX; ++i) t += fmax(xx[i] - ubx[i], 0.0); cl1 += t;
        return cl1;
    }
    // max_constraints_violation_impl :448-474 (maxima: order-free)
    __device__ double max_constraints_violation(const double* xx) const {
        Value ce[L::NE > 0 ? L::NE : 1], ci[L::NIL];
        ev.equalities(xx, ce);
        ev.inequalities(xx, ci);
        const double *lbg = at(L::LBG), *ubg = at(L::UBG), *lbx = at(L::LBX), *ubx = at(L::UBX);
        double c = 0.0;
        if (NE > 0) { for (int i = 0; i < NE; ++i) c = fmax(c, fabs(ce[i].v)); }
        if (NI > 0) {
            double a = -INFINITY, b = -INFINITY;
            for (int i = 0; i < NI; ++i) { a = fmax(a, lbg[i] - ci[i].v); b = fmax(b, ci[i].v - ubg[i]); }
            c = fmax(c, a); c = fmax(c, b);
        }
        double a = -INFINITY, b = -INFINITY;
        for (int i = 0; i < NX; ++i) { a = fmax(a, lbx[i] - xx[i]); b = fmax(b, xx[i] - ubx[i]); }
        c = fmax(c, a); c = fmax(c, b);
        return c;
    }
    // max |v_i| over count <= 64 entries, one per lane, from 0 as the checker's fmax fold (BoxADMM::inf_norm) starts: a NaN entry is
    // skipped, and a vector of NaNs has norm 0. The 0 seed matters at count = 64, where no idle lane contributes a 0 to the reduction.
    __device__ double inf_norm(const double* v, int count) const {
        const int ln = lane_id();
        const double a = fabs(v[ln < count ? ln : 0]);
        return fmax(0.0, wave_max(ln < count ? a : 0.0));
    }

    // ---- regularisation (sqp_test_autodiff.cpp:29-45, dense_sparse_compare.cpp:109-122) in the checker's form
    __device__ void rotate_cols(double* Am, int p, int q, double c, double sn) const {   // columns p, q of an NX x NX matrix, one row per lane
        const int k = lane_id();
        if (k < NX) { const double akp = Am[k + p * NX], akq = Am[k + q * NX]; Am[k + p * NX] = c * akp - sn * akq; Am[k + q * NX] = sn * akp + c * akq; }
        wsync();
    }
    __device__ void rotate_rows(double* Am, int p, int q, double c, double sn) const {
        const int k = lane_id();
        if (k < NX) { const double apk = Am[p + k * NX], aqk = Am[q + k * NX]; Am[p + k * NX] = c * apk - sn * aqk; Am[q + k * NX] = sn * apk + c * aqk; }
        wsync();
    }
    __device__ void rotation(double apq, double app, double aqq, double& c, double& sn) const {
        const double theta = (aqq - app) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + ::sqrt(theta * theta + 1));
        c = 1 / ::sqrt(t * t + 1); sn = t * c;
    }
    __device__ void jacobi_cyclic(double* Am, double* V) const {
        for (int sweep = 0; sweep < 100; ++sweep) {
            double off = 0;
            for (int i = 0; i < NX; ++i) for (int j = 0; j < i; ++j) off += Am[i + j * NX] * Am[i + j * NX];
            if (uniform(off < 1e-300)) break;
            for (int p = 0; p < NX; ++p)
                for (int q = p + 1; q < NX; ++q) {
                    const double apq = Am[p + q * NX];
                    if (uniform(fabs(apq) < 1e-300)) continue;
                    double c, sn; rotation(apq, Am[p + p * NX], Am[q + q * NX], c, sn);
                    wsync();
                    rotate_cols(Am, p, q, c, sn);
                    rotate_rows(Am, p, q, c, sn);
                    rotate_cols(V, p, q, c, sn);
                }
        }
    }
    __device__ void jacobi_round_robin(double* Am, double* V) const {
        constexpr int np = NX + (NX & 1), m2 = np / 2, nr = np - 1;
        double* cs = at(L::CS);
        auto pair_of = [&](int r, int i, int& p, int& q) {
            const int a = (i == 0) ? np - 1 : (r + i) % nr, b = (i == 0) ? r : (r - i + nr) % nr;
            p = a < b ? a : b; q = a < b ? b : a;
        };
        const int ln = lane_id();
        for (int sweep = 0; sweep < 100; ++sweep) {
            double amax = 0;
            for (int e = ln; e < NX * NX; e += WAVE) { const int i = e % NX, j = e / NX; if (i > j) amax = fmax(amax, fabs(Am[e])); }
            amax = wave_max(amax);
            if (uniform(amax * amax < 1e-300)) break;
            for (int r = 0; r < nr; ++r) {
                if (ln < m2) {   // the angles of every pair of the round from the matrix at its start
                    int p, q; pair_of(r, ln, p, q);
                    double c = 1.0, sn = 0.0;
                    if (q < NX) { const double apq = Am[p + q * NX]; if (!(fabs(apq) < 1e-300)) rotation(apq, Am[p + p * NX], Am[q + q * NX], c, sn); }
                    cs[ln] = c; cs[m2 + ln] = sn;
                }
                wsync();
                for (int i = 0; i < m2; ++i) {
                    int p, q; pair_of(r, i, p, q);
                    const double c = cs[i], sn = cs[m2 + i];
                    if (!uniform(q < NX && sn != 0.0)) continue;
                    rotate_cols(Am, p, q, c, sn);
                    rotate_cols(V, p, q, c, sn);
                }
                for (int i = 0; i < m2; ++i) {
                    int p, q; pair_of(r, i, p, q);
                    const double c = cs[i], sn = cs[m2 + i];
                    if (!uniform(q < NX && sn != 0.0)) continue;
                    rotate_rows(Am, p, q, c, sn);
                }
                if (ln == 0)
                    for (int i = 0; i < m2; ++i) {
                        int p, q; pair_of(r, i, p, q);
                        if (q < NX && cs[m2 + i] != 0.0) { Am[p + q * NX] = 0.0; Am[q + p * NX] = 0.0; }
                    }
                wsync();
            }
        }
    }
    __device__ void regularise_eig_mirror(double* H) const {
        double *Am = at(L::EA), *V = at(L::EV), *w = at(L::EW);
        const int ln = lane_id();
        for (int e = ln; e < NX * NX; e += WAVE) { Am[e] = H[e]; V[e] = (e % NX == e / NX) ? 1.0 : 0.0; }
        wsync();
        if constexpr (NX <= 8) jacobi_cyclic(Am, V); else jacobi_round_robin(Am, V);
        double mn = Am[0];
        for (int i = 1; i < NX; ++i) mn = fmin(mn, Am[i + i * NX]);
        if (!uniform(mn <= 0)) return;
        if (ln < NX) { double wi = Am[ln + ln * NX]; if (wi <= 0) wi = -1 * wi + 0.1; w[ln] = wi; }
        wsync();
        for (int e = ln; e < NX * NX; e += WAVE) {
            const int i = e % NX, j = e / NX;
            double a = 0;
            for (int k = 0; k < NX; ++k) a += (V[i + k * NX] * w[k]) * V[j + k * NX];
            H[e] = a;
        }
        wsync();
    }
    __device__ void regularise_gershgorin(double* H) const {   // column i touches its own diagonal entry only: one column per lane
        const int i = lane_id();
        if (i < NX) {
            const double aii = H[i + i * NX];
            double ri = 0; for (int k = 0; k < NX; ++k) ri += fabs(H[k + i * NX]);
            ri -= fabs(aii);
            if (aii - ri <= 0) H[i + i * NX] += (ri - aii) + 0.01;
        }
        wsync();
    }

    // ---- SQP steps
    __device__ void linearisation() {   // linearisation_dense_impl :310-318
        ev.first_order(at(L::X), at(L::LAM), at(L::H_), at(L::AL), at(L::A), at(L::LG));
        ev.hessian(at(L::X), at(L::LAM), at(L::HH));
        const int reg = __builtin_amdgcn_readfirstlane(ss.regularisation);
        if (reg == 1) regularise_eig_mirror(at(L::HH));
        else if (reg == 2) regularise_gershgorin(at(L::HH));
    }
    __device__ void bfgs_update(double* B, const double* sv, const double* y) {   // bfgs.hpp:23-52
        const int ln = lane_id();
        double* Bs = at(L::BS);
        double* r = at(L::RR);
        if (ln < NX) { double a = 0; for (int j = 0; j < NX; ++j) a += B[ln + j * NX] * sv[j]; Bs[ln] = a; }
        wsync();
        double sBs = 0, sy = 0;
        for (int i = 0; i < NX; ++i) sBs += sv[i] * Bs[i];
        for (int i = 0; i < NX; ++i) sy += sv[i] * y[i];
        double sr;
        const bool damp = sy < 0.2 * sBs;
        if (damp) {
            const double theta = 0.8 * sBs / (sBs - sy);
            if (ln < NX) r[ln] = theta * y[ln] + (1 - theta) * Bs[ln];
            sr = theta * sy + (1 - theta) * sBs;
        } else {
            if (ln < NX) r[ln] = y[ln];
            sr = sy;
        }
        wsync();
        if (uniform(sr < EPS)) return;
        for (int e = ln; e < NX * NX; e += WAVE) {
            const int i = e % NX, j = e / NX;
            double b = B[e];
            b += (-Bs[i] * Bs[j]) / sBs;
            b += (r[i] * r[j]) / sr;
            B[e] = b;
        }
        wsync();
    }
    __device__ void update_linearisation() {   // :490-504
        if (__builtin_amdgcn_readfirstlane(ss.exact_hessian_every_iter) != 0) { linearisation(); return; }
        double *lgn = at(L::LGN), *lg = at(L::LG);
        ev.first_order(at(L::X), at(L::LAM), at(L::H_), at(L::AL), at(L::A), lgn);
        double* yk = at(L::CS);   // y_k = new - previous Lagrangian gradient (the Jacobi angles' slot: free on this path)
        const int ln = lane_id();
        if (ln < NX) yk[ln] = lgn[ln] - lg[ln];
        wsync();
        bfgs_update(at(L::HH), at(L::STEP), yk);
        if (ln < NX) lg[ln] = lgn[ln];
        wsync();
    }
    __device__ void form_qp_bounds() {   // :588-593
        const int ln = lane_id();
        double *al = at(L::AL), *au = at(L::AU);
        if (ln < M) {
            double a = -al[ln];
            double u = a;
            if (ln >= NE) { a += at(L::LBG)[ln - NE]; u += at(L::UBG)[ln - NE]; }
            al[ln] = a; au[ln] = u;
        }
        if (ln < NX) { const double xv = at(L::X)[ln]; at(L::LX)[ln] = at(L::LBX)[ln] - xv; at(L::UX)[ln] = at(L::UBX)[ln] - xv; }
        wsync();
    }
    __device__ bool solve_qp() {   // :533-565; true when the QP gave up at its conditioning gate
        pmpc_qp_info qi;
        boxadmm_solve_reg<NX, M, false, true, true>(at(L::HH), at(L::H_), at(L::A), at(L::AL), at(L::AU), at(L::LX), at(L::UX), nullptr, nullptr, qs, qi,
                                                    at(L::PX), at(L::PY), at(L::TR));
        wsync();
        const bool gave_up = uniform((qi.flags & PMPC_FLAG_ILLCOND) != 0);
        // a gate trip at a refactorisation: the register QP has already counted the ADMM iteration that asked for the new rho (it advances
        // its counter before it refactorises), the checker reports that iteration itself as the one the QP stopped at
        qp_iter_total += (gave_up && qi.iter > 1) ? qi.iter - 1 : qi.iter;
        qp_flags |= qi.flags;
        return gave_up;
    }
    __device__ double step_size_selection() {   // :380-419
        const double *x = at(L::X), *p = at(L::PX), *h = at(L::H_);
        double* xs = at(L::XS);
        const int ln = lane_id();
        const double constr_l1 = constraints_violation(x);
        const double mu = inf_norm(at(L::LAMK), M + NX);
        const double cost_1 = ev.cost(x);
        const double phi_l1 = cost_1 + mu * constr_l1;
        double gp = 0; for (int i = 0; i < NX; ++i) gp += h[i] * p[i];
        const double Dp_phi_l1 = gp - mu * constr_l1;
        double alpha = 1.0;
        for (int i = 1; i < ss.line_search_max_iter; ++i) {
            if (ln < NX) { double t = alpha * p[ln]; t += x[ln]; xs[ln] = t; }
            wsync();
            const double cost_step = ev.cost(xs);
            cost_log = cost_step;
            const double phi_step = cost_step + mu * constraints_violation(xs);
            if (uniform(phi_step <= (phi_l1 + alpha * ss.eta * Dp_phi_l1))) return alpha;
            alpha = ss.tau * alpha;
        }
        return alpha;
    }
    __device__ void iterate_tail() {
        const int ln = lane_id();
        double *py = at(L::PY), *lam = at(L::LAM), *lamk = at(L::LAMK), *px = at(L::PX), *x = at(L::X);
        if (ln < M + NX) { const double v = py[ln]; lamk[ln] = v; py[ln] = v - lam[ln]; }
        wsync();
        const double alpha = step_size_selection();
        wsync();
        if (ln < NX) { x[ln] += alpha * px[ln]; at(L::STEP)[ln] = alpha * px[ln]; }
        if (ln < M + NX) lam[ln] += alpha * py[ln];
        wsync();
        primal_norm = alpha * inf_norm(px, NX);
        dual_norm = alpha * inf_norm(py, M + NX);
    }
    __device__ bool termination_criteria() {   // :524-529
        max_violation = max_constraints_violation(at(L::X));
        return uniform((primal_norm <= ss.eps_prim) && (dual_norm <= ss.eps_dual) && (max_violation <= ss.eps_prim));
    }
    // solve :569-696 -> (iter, status)
    __device__ void solve(int& iter, int& status) {
        status = PMPC_SQP_MAX_ITER_EXCEEDED;
        iter = 1;
        linearisation();
        form_qp_bounds();
        if (solve_qp()) { status = PMPC_NLP_ILLCOND_STOP; return; }
        iterate_tail();
        if (termination_criteria()) { status = PMPC_SQP_SOLVED; return; }
        while (iter < ss.max_iter) {
            ++iter;
            update_linearisation();
            form_qp_bounds();
            if (solve_qp()) { status = PMPC_NLP_ILLCOND_STOP; return; }
            iterate_tail();
            if (termination_criteria()) { status = PMPC_SQP_SOLVED; break; }
        }
    }
};

// One instance per 64-lane workgroup. Inputs may be null (x_guess, lam_guess, d: zeros; lbx, lbg: -inf; ubx, ubg: +inf).
template <class Def>
__global__ __launch_bounds__(64) void nlp_kernel(Def def, int B, const double* __restrict__ x_guess, const double* __restrict__ lam_guess,
                                                 const double* __restrict__ d, const double* __restrict__ lbx, const double* __restrict__ ubx,
                                                 const double* __restrict__ lbg, const double* __restrict__ ubg, pmpc_sqp_settings ss,
                                                 pmpc_qp_settings qs, double* __restrict__ x, double* __restrict__ lam, pmpc_sqp_info* __restrict__ info) {
    using L = NlpLayout<Def>;
    constexpr int NX = L::NX, M = L::M, NI = L::NI, NP = L::NP;
    extern __shared__ double smem[];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int ln = lane_id();
    double* s = smem;
    if (ln < NX) {
        const size_t k = (size_t)b * NX + ln;
        s[L::X + ln] = x_guess ? x_guess[k] : 0.0;
        s[L::LBX + ln] = lbx ? lbx[k] : -INFINITY;
        s[L::UBX + ln] = ubx ? ubx[k] : INFINITY;
    }
    if (ln < M + NX) s[L::LAM + ln] = lam_guess ? lam_guess[(size_t)b * (M + NX) + ln] : 0.0;
    if (ln < NI) {
        s[L::LBG + ln] = lbg ? lbg[(size_t)b * NI + ln] : -INFINITY;
        s[L::UBG + ln] = ubg ? ubg[(size_t)b * NI + ln] : INFINITY;
    }
    for (int i = ln; i < NP; i += WAVE) s[L::PAR + i] = d ? d[(size_t)b * NP + i] : 0.0;
    wsync();
    NlpSqp<Def> sqp{NlpEval<Def>{def, s + L::PAR}, s, ss, qs};
    int iter, status;
    sqp.solve(iter, status);
    wsync();
    const double xv = s[L::X + (ln < NX ? ln : 0)], lv = s[L::LAM + (ln < M + NX ? ln : 0)];
    if (ln < NX) x[(size_t)b * NX + ln] = xv;
    if (ln < M + NX) lam[(size_t)b * (M + NX) + ln] = lv;
    const bool bad = __builtin_amdgcn_ballot_w64(((ln < NX) && (xv - xv) != 0.0) || ((ln < M + NX) && (lv - lv) != 0.0)) != 0;
    if (ln == 0) {
        pmpc_sqp_info r;
        r.iter = iter; r.qp_solver_iter = sqp.qp_iter_total; r.status = status; r.flags = sqp.qp_flags | (bad ? PMPC_FLAG_NONFINITE : 0);
        r.primal_norm = sqp.primal_norm; r.dual_norm = sqp.dual_norm; r.max_violation = sqp.max_violation; r.cost = sqp.cost_log;
        info[b] = r;
    }
}

// GenericNLP::lagrangian_gradient_hessian at B points: cost, constraint values [eq | ineq], Jacobian (M x NX column-major), cost gradient,
// Lagrangian gradient, Lagrangian Hessian (NX x NX column-major). Any output may be null.
template <class Def>
__global__ __launch_bounds__(64) void nlp_linearise_kernel(Def def, int B, const double* __restrict__ xin, const double* __restrict__ lamin,
                                                           const double* __restrict__ d, double* cost, double* constr, double* jac, double* cost_grad,
                                                           double* lag_grad, double* lag_hess) {
    using L = NlpLayout<Def>;
    constexpr int NX = L::NX, M = L::M, NP = L::NP;
    extern __shared__ double smem[];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int ln = lane_id();
    double* s = smem;
    if (ln < NX) s[L::X + ln] = xin[(size_t)b * NX + ln];
    if (ln < M + NX) s[L::LAM + ln] = lamin ? lamin[(size_t)b * (M + NX) + ln] : 0.0;
    for (int i = ln; i < NP; i += WAVE) s[L::PAR + i] = d ? d[(size_t)b * NP + i] : 0.0;
    wsync();
    NlpEval<Def> ev{def, s + L::PAR};
    const double c = ev.first_order(s + L::X, s + L::LAM, s + L::H_, s + L::AL, s + L::A, s + L::LG);
    ev.hessian(s + L::X, s + L::LAM, s + L::HH);
    if (cost && ln == 0) cost[b] = c;
    if (constr && ln < M) constr[(size_t)b * M + ln] = s[L::AL + ln];
    if (cost_grad && ln < NX) cost_grad[(size_t)b * NX + ln] = s[L::H_ + ln];
    if (lag_grad && ln < NX) lag_grad[(size_t)b * NX + ln] = s[L::LG + ln];
    for (int e = ln; e < M * NX; e += WAVE) if (jac) jac[(size_t)b * M * NX + e] = s[L::A + e];
    for (int e = ln; e < NX * NX; e += WAVE) if (lag_hess) lag_hess[(size_t)b * NX * NX + e] = s[L::HH + e];
}

// settings this route implements: the defaults of every policy hook (pmpc_sqp_settings), regularisation 0 / 1 / 2
inline pmpc_status nlp_check_settings(const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs) {
    if (ss->hessian_update != 0 || ss->qp_solver != 0 || ss->preconditioner != 0 || ss->line_search != 0 || ss->kkt_form != 0 ||
        ss->filter_state != nullptr || ss->iteration_trace != nullptr || ss->regularisation < 0 || ss->regularisation > 2 || qs->linear_solver != 0)
        return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

template <class Def>
pmpc_status nlp_launch_dev(pmpc_context* ctx, const Def& def, int B, const double* x_guess, const double* lam_guess, const double* d,
                           const double* lbx, const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                           const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    using L = NlpLayout<Def>;
    if (!ctx || B < 0 || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status chk = nlp_check_settings(ss, qs);
    if (chk != PMPC_OK) return chk;
    if constexpr (!L::FITS) {
        return PMPC_ERR_UNSUPPORTED_SIZE;   // more than 64 KKT rows: no route yet
    } else {
        if (B == 0) return PMPC_OK;
        void* stream = nullptr; size_t lds_limit = 0;
        const pmpc_status st = pmpc_internal_nlp_services(ctx, &stream, &lds_limit);
        if (st != PMPC_OK) return st;
        const size_t lds = L::lds_bytes(ss->regularisation);
        if (lds > lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
        if (hipFuncSetAttribute((const void*)nlp_kernel<Def>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return PMPC_ERR_HIP;
        hipLaunchKernelGGL(nlp_kernel<Def>, dim3(B), dim3(WAVE), lds, (hipStream_t)stream, def, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, *ss, *qs,
                           x, lam, info);
        return hipGetLastError() == hipSuccess ? PMPC_OK : PMPC_ERR_HIP;
    }
}

template <class Def>
pmpc_status nlp_linearise_dev(pmpc_context* ctx, const Def& def, int B, const double* xin, const double* lamin, const double* d, double* cost,
                              double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    using L = NlpLayout<Def>;
    if (!ctx || B < 0 || (B > 0 && !xin)) return PMPC_ERR_INVALID_ARGUMENT;
    if constexpr (!L::FITS) {
        return PMPC_ERR_UNSUPPORTED_SIZE;
    } else {
        if (B == 0) return PMPC_OK;
        void* stream = nullptr; size_t lds_limit = 0;
        const pmpc_status st = pmpc_internal_nlp_services(ctx, &stream, &lds_limit);
        if (st != PMPC_OK) return st;
        const size_t lds = L::lds_bytes(0);
        if (lds > lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
        if (hipFuncSetAttribute((const void*)nlp_linearise_kernel<Def>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return PMPC_ERR_HIP;
        hipLaunchKernelGGL(nlp_linearise_kernel<Def>, dim3(B), dim3(WAVE), lds, (hipStream_t)stream, def, B, xin, lamin, d, cost, constr, jac, cost_grad,
                           lag_grad, lag_hess);
        return hipGetLastError() == hipSuccess ? PMPC_OK : PMPC_ERR_HIP;
    }
}

}  // namespace pmpc
