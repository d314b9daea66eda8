// polympc_amd — the active-set KKT solve of a QP (the operation: include/polympc_amd.h, "polish"): one 64-lane wavefront per instance, the
// reduced KKT matrix and its right-hand sides column-major in LDS with lanes <-> rows, so that a row update touches 64 consecutive doubles (no
// bank conflict on the 64 x 4 B banks: two passes of 32 lanes each) and the read of the pivot row's entry is one broadcast. Gaussian elimination
// with partial pivoting carries the right-hand sides along; no factor is kept. The pivot search is a wave reduction over (key, row).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/polympc_amd.h"

namespace pmpc {

constexpr int POLISH_LANES = 64;

struct PolishArgs {
    int B, n, m, frozen, nsens;
    int sens[PMPC_POLISH_MAX_SENS];
    double act_tol;
    const double *H, *h, *A, *Alb, *Aub, *xlb, *xub, *p_in, *y_in;
    signed char* masks;
    double *p, *y;
    pmpc_polish_info* info;
    double* dP;
};

// LDS of one instance: N x (N + 1 + nsens) doubles of [K | b | sensitivity columns], the targets and the point (N doubles each), the masks (N ints)
__host__ __device__ inline size_t polish_lds_bytes(int n, int m, int nsens) {
    const size_t N = (size_t)n + (size_t)m;
    return 8 * N * (N + 1 + (size_t)nsens) + 20 * N + 4 * (N & 1);   // (padded to whole doubles)
}

__device__ inline double polish_key(double v) { v = fabs(v); return v != v ? (double)INFINITY : v; }   // a NaN counts as +inf
__device__ inline bool polish_finite(double v) { return fabs(v) < (double)INFINITY; }                  // (false for a NaN)
__device__ inline double polish_wave_max(double v) {
    for (int off = 1; off < POLISH_LANES; off <<= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}
__device__ inline int polish_wave_count(bool pred) { return __popcll(__ballot(pred)); }

__global__ __launch_bounds__(POLISH_LANES) void polish_kernel(PolishArgs a) {
    extern __shared__ double polish_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, m = a.m, N = n + m, R = 1 + a.nsens, NC = N + R;
    double* K = polish_lds;                  // column-major, N rows: columns 0 .. N-1 the matrix, N the right-hand side, N+1 .. the sensitivity columns
    double* tv = K + (size_t)N * NC;         // targets, variables first, then rows (the order of z)
    double* pv = tv + N;                     // p_in on variables, A p_in on rows
    int* mk = (int*)(pv + N);                // masks in the same order
    const double* H = a.H + (size_t)b * n * n; const double* h = a.h + (size_t)b * n;
    const double* A = a.A + (size_t)b * m * n; const double* Alb = a.Alb + (size_t)b * m; const double* Aub = a.Aub + (size_t)b * m;
    const double* xlb = a.xlb + (size_t)b * n; const double* xub = a.xub + (size_t)b * n;
    const double* p_in = a.p_in ? a.p_in + (size_t)b * n : nullptr;
    const double* y_in = a.y_in ? a.y_in + (size_t)b * N : nullptr;
    signed char* masks = a.masks + (size_t)b * N;
    const double tol = a.act_tol;
    auto Hs = [&](int i, int j) { return i >= j ? H[i + (size_t)n * j] : H[j + (size_t)n * i]; };   // the lower triangle, mirrored

    // ---- 1. the point and the active set
    for (int i = lane; i < n; i += POLISH_LANES) pv[i] = p_in ? p_in[i] : 0.0;
    __syncthreads();
    int n_av = 0, n_ar = 0;
    for (int e0 = 0; e0 < N; e0 += POLISH_LANES) {
        const int e = e0 + lane;
        int mask = 0;
        if (e < N) {
            double lo, hi, v;
            if (e < n) { lo = xlb[e]; hi = xub[e]; v = pv[e]; }
            else {
                const int r = e - n;
                lo = Alb[r]; hi = Aub[r]; v = 0.0;
                for (int j = 0; j < n; ++j) v = v + A[r + (size_t)m * j] * pv[j];
            }
            const double dl = v - lo, du = hi - v;
            if (a.frozen) mask = (int)masks[e < n ? m + e : e - n] & 3;
            else {
                const bool eq = hi - lo < 1e-4, al = polish_finite(lo) && dl <= tol, au = polish_finite(hi) && du <= tol;
                mask = eq ? 3 : (au && (!al || du < dl)) ? 2 : al ? 1 : 0;
                masks[e < n ? m + e : e - n] = (signed char)mask;
            }
            tv[e] = (mask == 2 || (mask == 3 && du < dl)) ? hi : lo;
            if (e >= n) pv[e] = v;
            mk[e] = mask;
        }
        n_av += polish_wave_count(e < n && mask != 0);
        n_ar += polish_wave_count(e >= n && e < N && mask != 0);
    }
    __syncthreads();

    // ---- 2. the reduced system, its right-hand side, the sensitivity columns; the residual of the input
    int flags = 0;
    for (int c = 0; c < N; ++c) {
        const int mc = mk[c];
        for (int e = lane; e < N; e += POLISH_LANES) {
            const int me = mk[e];
            double v;
            if (c < n) {
                if (e < n) v = (me == 0 && mc == 0) ? Hs(e, c) : (e == c ? 1.0 : 0.0);
                else v = (me != 0 && mc == 0) ? A[(e - n) + (size_t)m * c] : 0.0;
            } else {
                if (e < n) v = (mc != 0 && me == 0) ? A[(c - n) + (size_t)m * e] : 0.0;
                else v = (e == c && me == 0) ? 1.0 : 0.0;
            }
            K[(size_t)c * N + e] = v;
        }
    }
    double res = 0.0;
    for (int e = lane; e < N; e += POLISH_LANES) {
        const int me = mk[e];
        double bv, term;
        if (e < n) {
            if (me == 0) {
                bv = -h[e];
                for (int j = 0; j < n; ++j) if (mk[j] != 0) bv = bv - Hs(e, j) * tv[j];
                double g = 0.0;
                for (int j = 0; j < n; ++j) g = g + Hs(e, j) * pv[j];
                g = g + h[e];
                double s = 0.0;
                for (int r = 0; r < m; ++r) s = s + A[r + (size_t)m * e] * ((y_in && mk[n + r] != 0) ? y_in[r] : 0.0);
                g = g + s;
                term = polish_key(g);
            } else { bv = tv[e]; term = polish_key(pv[e] - tv[e]); }
        } else if (me != 0) {
            const int r = e - n;
            bv = tv[e];
            for (int j = 0; j < n; ++j) if (mk[j] != 0) bv = bv - A[r + (size_t)m * j] * tv[j];
            term = polish_key(pv[e] - tv[e]);
        } else { bv = 0.0; term = 0.0; }
        K[(size_t)N * N + e] = bv;
        res = term > res ? term : res;
    }
    res = polish_wave_max(res);
    for (int q = 0; q < a.nsens; ++q) {
        const int j = a.sens[q];
        const bool valid = j >= 0 && j < n && mk[j < 0 || j >= n ? 0 : j] == 3;
        if (!valid) flags |= PMPC_POLISH_SENS_INACTIVE;
        for (int e = lane; e < N; e += POLISH_LANES) {
            const int me = mk[e];
            double v = 0.0;
            if (valid) {
                if (e < n) v = me == 0 ? -Hs(e, j) : (e == j ? 1.0 : 0.0);
                else if (me != 0) v = -A[(e - n) + (size_t)m * j];
            }
            K[(size_t)(N + 1 + q) * N + e] = v;
        }
    }
    __syncthreads();

    // ---- 3. elimination with partial pivoting, the right-hand sides carried along
    double pmin = (double)INFINITY, pmax = 0.0;
    bool singular = false;
    for (int k = 0; k < N; ++k) {
        double* col = K + (size_t)k * N;
        double bk = -1.0; int bi = 0x7fffffff;
        for (int r = lane; r < N; r += POLISH_LANES)
            if (r >= k) { const double key = polish_key(col[r]); if (key > bk) { bk = key; bi = r; } }
        for (int off = 1; off < POLISH_LANES; off <<= 1) {
            const double ok = __shfl_xor(bk, off); const int oi = __shfl_xor(bi, off);
            if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        if (!(bk > 0.0) || !polish_finite(bk)) { singular = true; break; }   // (uniform: every lane holds the same pair)
        pmin = bk < pmin ? bk : pmin; pmax = bk > pmax ? bk : pmax;
        if (bi != k) {
            for (int c = k + lane; c < NC; c += POLISH_LANES) {
                const double u = K[(size_t)c * N + k]; K[(size_t)c * N + k] = K[(size_t)c * N + bi]; K[(size_t)c * N + bi] = u;
            }
            __syncthreads();
        }
        const double piv = col[k];
        for (int r = lane; r < N; r += POLISH_LANES) {
            if (r <= k) continue;
            const double l = col[r] / piv;
            for (int c = k + 1; c < NC; ++c) K[(size_t)c * N + r] = K[(size_t)c * N + r] - l * K[(size_t)c * N + k];
        }
        __syncthreads();
    }

    pmpc_polish_info* info = a.info + b;
    if (singular) {
        if (lane == 0) { info->active_vars = n_av; info->active_rows = n_ar; info->flags = flags | PMPC_POLISH_SINGULAR; info->reserved = 0;
                         info->res_in = res; info->pivot_min = 0.0; info->pivot_max = pmax; }
        return;
    }

    // ---- back substitution, every right-hand side
    for (int k = N - 1; k >= 0; --k) {
        const double* col = K + (size_t)k * N;
        if (lane == (k & (POLISH_LANES - 1)))
            for (int q = 0; q < R; ++q) { double* bq = K + (size_t)(N + q) * N; bq[k] = bq[k] / col[k]; }
        __syncthreads();
        for (int q = 0; q < R; ++q) {
            double* bq = K + (size_t)(N + q) * N;
            const double zk = bq[k];
            for (int r = lane; r < k; r += POLISH_LANES) bq[r] = bq[r] - col[r] * zk;
        }
        __syncthreads();
    }

    // ---- 4. outputs
    const double* z = K + (size_t)N * N;
    double* p = a.p + (size_t)b * n; double* y = a.y + (size_t)b * N;
    bool sign = false, infeas = false, nonfin = false;
    for (int e0 = 0; e0 < N; e0 += POLISH_LANES) {
        const int e = e0 + lane;
        if (e < N) {
            const int me = mk[e];
            double lo, hi, v, mult;
            if (e < n) {
                lo = xlb[e]; hi = xub[e]; v = z[e];
                double g = 0.0;
                for (int j = 0; j < n; ++j) g = g + Hs(e, j) * z[j];
                g = g + h[e];
                double s = 0.0;
                for (int r = 0; r < m; ++r) s = s + A[r + (size_t)m * e] * (mk[n + r] != 0 ? z[n + r] : 0.0);
                g = g + s;
                mult = me != 0 ? -g : 0.0;
                p[e] = v; y[m + e] = mult;
                nonfin = nonfin || !polish_finite(v);
            } else {
                const int r = e - n;
                lo = Alb[r]; hi = Aub[r]; v = 0.0;
                for (int j = 0; j < n; ++j) v = v + A[r + (size_t)m * j] * z[j];
                mult = me != 0 ? z[e] : 0.0;
                y[r] = mult;
            }
            nonfin = nonfin || !polish_finite(mult);
            sign = sign || (me == 1 && mult > 0.0) || (me == 2 && mult < 0.0);
            infeas = infeas || (me != 1 && me != 3 && lo - v > tol) || (me != 2 && me != 3 && v - hi > tol);
        }
    }
    for (int q = 0; q < a.nsens; ++q) {
        const int j = a.sens[q];
        const bool valid = j >= 0 && j < n && mk[j < 0 || j >= n ? 0 : j] == 3;
        const double* zq = K + (size_t)(N + 1 + q) * N;
        double* dp = a.dP + ((size_t)b * a.nsens + q) * n;
        for (int i = lane; i < n; i += POLISH_LANES) dp[i] = valid ? zq[i] : 0.0;
    }
    if (__any(sign)) flags |= PMPC_POLISH_SIGN;
    if (__any(infeas)) flags |= PMPC_POLISH_INFEASIBLE;
    if (__any(nonfin)) flags |= PMPC_POLISH_NONFINITE;
    if (lane == 0) { info->active_vars = n_av; info->active_rows = n_ar; info->flags = flags; info->reserved = 0;
                     info->res_in = res; info->pivot_min = pmin; info->pivot_max = pmax; }
}

}  // namespace pmpc
