// polympc_amd — the interpolant of a stored trajectory on the device (pmpc_traj.hip): x(t) / u(t) sampling, the time-shifted warm start and the
// change of grid are one operation — evaluate the piecewise Lagrange interpolant of the per-node blocks of an iterate at a set of times. It restates
// MPC<OCP>::interpolate of the host mirror (include/polympc/polympc.hpp; LagrangeSpline::eval as mpc_wrapper.hpp:245-281 calls it): the segment
// is located by t / L, and the basis of the FIRST segment is evaluated, in product form, at the local time. Every output element is one serial
// chain of IEEE operations in a fixed order (the library is built with -ffp-contract=off), so a result does not depend on the launch geometry:
//   idx = clamp((int)floor(t / L), 0, S - 1);  tl = t - idx * L
//   l_i = 1; for j = 0..P, j != i: l_i = l_i * ((tl - s_j) / (s_i - s_j))           s_j: forward node j of the first segment
//   r   = 0; for i = 0..P:         r   = r + l_i * v_{idx P + i}                    v_k: the value at FORWARD node k = storage node nn - 1 - k
#pragma once
#include <hip/hip_runtime.h>
#include "pmpc_ocp.hpp"

namespace pmpc {

constexpr int TRAJ_CHUNK = 4;        // target times per workgroup of the sampling / regridding kernel: 4 x (MAX_P + 1) weights = one per lane
constexpr int TRAJ_MAX_BLOCKS = 6;   // per-node blocks of a shift: x, u and the four dual blocks

// the source grid, passed by value
struct TrajGrid {
    int P, S, nn, _pad;
    double L;               // segment length (tf - t0) / S
    double s[MAX_P + 1];    // forward nodes of the first segment: s[j] = tn[nn - 1 - j]
};
// target times of a shift / a regrid: forward node k of the target at t[k]
struct TrajTimes { double t[MAX_NODES]; };

// The per-node blocks a shift moves. Block k holds component c of storage node s at off[k] + s * nc[k] + c of its instance row — of the primal row
// (in_lam[k] = 0) or of the dual row (1); end[k] is the running number of components per node.
struct TrajBlocks {
    int count = 0;
    int off[TRAJ_MAX_BLOCKS], nc[TRAJ_MAX_BLOCKS], end[TRAJ_MAX_BLOCKS], in_lam[TRAJ_MAX_BLOCKS];
    void add(int offset, int comps, int lam) {
        if (comps <= 0 || count >= TRAJ_MAX_BLOCKS) return;
        off[count] = offset; nc[count] = comps; in_lam[count] = lam; end[count] = (count ? end[count - 1] : 0) + comps;
        ++count;
    }
    __host__ __device__ int comps() const { return count ? end[count - 1] : 0; }
};

// segment of t and the local time (a NaN or a time before the horizon takes the first segment, a time past it the last)
__device__ inline int traj_locate(double t, double L, int S, double& tl) {
    const double f = floor(t / L);
    const int idx = !(f > 0.0) ? 0 : (f < (double)(S - 1) ? (int)f : S - 1);
    tl = t - idx * L;
    return idx;
}

__device__ inline double traj_weight(const double* s, int P, double tl, int i) {
    const double si = s[i];
    double l = 1.0;
    for (int j = 0; j <= P; ++j)
        if (j != i) l = l * ((tl - s[j]) / (si - s[j]));
    return l;
}

// The basis of `count` target times, shared by all components: w[q (P + 1) + i] = l_i of time q, seg[q] = its segment. One weight per lane and pass.
template <class TimeAt>
__device__ inline void traj_basis(const TrajGrid& g, int count, TimeAt time_at, double* w, int* seg, int lane) {
    const int np1 = g.P + 1;
    for (int it = lane; it < count * np1; it += 64) {
        const int q = it / np1, i = it - q * np1;
        double tl;
        const int idx = traj_locate(time_at(q), g.L, g.S, tl);
        w[it] = traj_weight(g.s, g.P, tl, i);
        if (i == 0) seg[q] = idx;
    }
}

// One (instance, target time, component) of a per-node block with nc components per node: l = the time's weights, v = the component at forward
// node idx * P. Storage runs backwards in time, so forward node k + 1 lies nc doubles BELOW forward node k.
__device__ inline double traj_combine(const double* l, int P, const double* v, int nc) {
    double r = 0.0;
    for (int i = 0; i <= P; ++i) r = r + l[i] * v[-(long long)i * nc];
    return r;
}

}  // namespace pmpc
