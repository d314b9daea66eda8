// polympc_amd — the plant of a closed loop on the device (pmpc_plant.hip, and PMPC_REGISTER_OCP in a user's translation unit): one control period of
// x' = f(x, u, p, d, t) integrated with the OCP's own dynamics_impl, instantiated with pmpc::Value — the value-only scalar of the line search, so
// every transcendental is the one of pmpc_math.hpp. One lane per instance. Every state component is one serial chain of IEEE operations in a
// fixed order (the library is built with -ffp-contract=off), so a result does not depend on the launch geometry:
//   h = dt / substeps
//   for s = 0 .. substeps - 1:  ts = (double)s * h
//     Euler: k1 = f(x, u(ts), t0 + ts);             x_i = x_i + h * k1_i
//     RK4:   k1 = f(x, u(ts), t0 + ts)
//            xa_i = x_i + (0.5 * h) * k1_i;         k2 = f(xa, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
//            xb_i = x_i + (0.5 * h) * k2_i;         k3 = f(xb, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
//            xc_i = x_i + h * k3_i;                 k4 = f(xc, u(ts + h), t0 + (ts + h))
//            x_i = x_i + (h / 6.0) * (((k1_i + 2.0 * k2_i) + 2.0 * k3_i) + k4_i)
//   after the last substep, if w is given: x_i = x_i + w_i
// u(tau): the given u0 (control = 0), or the interpolant of the instance's iterate (control = 1; pmpc_traj.hpp, unchanged). ts + h of one substep and
// (double)(s + 1) * h of the next need not be the same bits, so the basis is kept per STAGE: 3 times per RK4 substep, 1 per Euler substep.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/polympc_amd.h"
#include "pmpc_traj.hpp"

namespace pmpc {

constexpr int PLANT_MAX_SUBSTEPS = 64;
constexpr int PLANT_LANES = 64;   // instances per workgroup

struct PlantArgs {
    TrajGrid g;                       // the controller's grid (control = 1)
    int integrator, substeps, control, B;
    double t0, dt;
    size_t n;                         // length of an iterate row
    double* state;                    // B * NX, in place
    const double *u0, *iterate, *d, *w;
};
constexpr int PLANT_REG_NX = 8;   // models of more states keep what the model reads and writes by index in LDS: their dynamics index the vectors in
                                  // loops that the compiler does not unroll, which would put per-lane arrays into scratch
// one lane's row of such a model: [argument nx | result nx | u nu | p np], an odd number of doubles, so that the 32 lanes of a ds_read_b64 group
// fall on 32 different bank pairs
__host__ __device__ constexpr int plant_row_doubles(int nx, int nu, int np) { return (2 * nx + nu + np) | 1; }
// stage times of a step, and the dynamic LDS of a launch: [weights stages (P + 1) | segments stages ints | pad to 16 bytes | nx > PLANT_REG_NX: 64 rows]
__host__ __device__ inline int plant_stages(int integrator, int substeps, int control) { return control == 1 ? substeps * (integrator == 1 ? 3 : 1) : 0; }
__host__ __device__ inline size_t plant_basis_bytes(int P, int stages) {
    return ((size_t)stages * (P + 1) * sizeof(double) + (size_t)stages * sizeof(int) + 15) & ~(size_t)15;
}
inline size_t plant_lds_bytes(int nx, int nu, int np, int P, int integrator, int substeps, int control) {
    return plant_basis_bytes(P, plant_stages(integrator, substeps, control)) +
           (nx > PLANT_REG_NX ? (size_t)PLANT_LANES * plant_row_doubles(nx, nu, np) * sizeof(double) : 0);
}

// Lane l of workgroup g integrates instance 64 g + l. The control basis of the stage times is the same for the whole batch: one weight per lane and
// pass into LDS. The body runs at full EXEC — the lanes past the batch redo the last instance — and only the final stores are predicated.
template <class Model>
__global__ __launch_bounds__(PLANT_LANES) void plant_kernel(Model model, PlantArgs a) {
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP, ND = Model::ND;
    extern __shared__ __attribute__((aligned(16))) double plant_lds[];
    const int lane = threadIdx.x, P = a.g.P, np1 = P + 1, nn = a.g.nn;
    const int per = a.integrator == 1 ? 3 : 1, stages = plant_stages(a.integrator, a.substeps, a.control);
    const double h = a.dt / (double)a.substeps, hh = 0.5 * h;
    double* wgt = plant_lds;
    int* seg = (int*)(wgt + stages * np1);
    traj_basis(a.g, stages, [&](int q) {
        const int s = q / per, j = q - s * per;
        const double ts = (double)s * h;
        return j == 0 ? ts : (j == 1 ? ts + hh : ts + h);
    }, wgt, seg, lane);
    __syncthreads();

    const size_t gid = (size_t)blockIdx.x * PLANT_LANES + lane;
    const size_t b = gid < (size_t)a.B ? gid : (size_t)a.B - 1;
    constexpr bool IN_LDS = NX > PLANT_REG_NX;
    Value x[NX], acc[NX], xs_reg[IN_LDS ? 1 : NX], k_reg[IN_LDS ? 1 : NX], u_reg[IN_LDS || NU == 0 ? 1 : NU], p_reg[IN_LDS || NP == 0 ? 1 : NP];
    Value *xs = xs_reg, *k = k_reg, *u = u_reg, *p = p_reg;   // the model's argument (when it is not x itself), its result, the control, the parameters
    if constexpr (IN_LDS) {
        xs = reinterpret_cast<Value*>(reinterpret_cast<char*>(plant_lds) + plant_basis_bytes(P, stages)) + (size_t)lane * plant_row_doubles(NX, NU, NP);
        k = xs + NX; u = k + NX; p = u + NU;
    }
    double dl[ND > 0 ? ND : 1];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = Value(a.state[b * NX + i]);
#pragma unroll
    for (int i = 0; i < NP; ++i) p[i] = Value(a.iterate[b * a.n + (size_t)(NX + NU) * nn + i]);
#pragma unroll
    for (int i = 0; i < ND; ++i) dl[i] = a.d[b * ND + i];
    if (a.control == 0) {
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = Value(a.u0[b * NU + i]);
    }
    const double* ub = a.control == 1 ? a.iterate + b * a.n + (size_t)NX * nn : nullptr;   // the instance's u block
    auto control_at = [&](int q) {   // u <- the interpolant at stage time q
        if (a.control != 1) return;
        const size_t top = (size_t)(nn - 1 - seg[q] * P);   // storage node of forward node idx P; the chain ends at storage node top - P >= 0
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = Value(traj_combine(wgt + q * np1, P, ub + top * NU + c, NU));
    };
    auto f = [&](const Value* at, double t, Value* out) {
#pragma unroll
        for (int i = 0; i < NX; ++i) out[i] = Value(0.0);
        model.template dynamics_impl<Value>(cref<Value>(at), cref<Value>(u), cref<Value>(p), cref<double>(dl), Value(t), vref<Value>(out));
    };
    for (int s = 0; s < a.substeps; ++s) {
        const double ts = (double)s * h;
        control_at(s * per);
        if constexpr (IN_LDS) {
#pragma unroll
            for (int i = 0; i < NX; ++i) xs[i] = x[i];
            f(xs, a.t0 + ts, k);
        } else {
            f(x, a.t0 + ts, k);
        }
        if (a.integrator == 0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i].v = x[i].v + h * k[i].v;
            continue;
        }
        const double tm = ts + hh, te = ts + h;
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i] = k[i]; xs[i].v = x[i].v + hh * k[i].v; }
        control_at(s * per + 1);
        f(xs, a.t0 + tm, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i].v = acc[i].v + 2.0 * k[i].v; xs[i].v = x[i].v + hh * k[i].v; }
        f(xs, a.t0 + tm, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i].v = acc[i].v + 2.0 * k[i].v; xs[i].v = x[i].v + h * k[i].v; }
        control_at(s * per + 2);
        f(xs, a.t0 + te, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i].v = x[i].v + (h / 6.0) * (acc[i].v + k[i].v);
    }
    if (a.w) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i].v = x[i].v + a.w[b * NX + i];
    }
    if (gid < (size_t)a.B) {
#pragma unroll
        for (int i = 0; i < NX; ++i) a.state[b * NX + i] = x[i].v;
    }
}

}  // namespace pmpc

// The library's part of a launch (pmpc_plant.hip): every argument check of the plant entries, made before any device call, then the device, the
// poison harness, the grid and the stream. blocks == 0 on return: nothing to launch (an empty batch, or a refusal).
extern "C" pmpc_status pmpc_internal_plant_prepare(pmpc_context* ctx, int nx, int nu, int np, int nd, int P, int S, double t0, double tf, int B, double dt,
                                                   const pmpc_plant_settings* settings, double* state, const double* u0, const double* iterate,
                                                   const double* d, const double* w, pmpc::PlantArgs* args, unsigned* blocks, size_t* lds, void** stream);

namespace pmpc {

// pmpc_plant_dev_fn of the OCP `Model`: the built-in models (pmpc_plant.hip) and PMPC_REGISTER_OCP
template <class Model>
inline pmpc_status plant_launch_dev(pmpc_context* ctx, const Model& model, int P, int S, double t0, double tf, int B, double dt,
                                    const pmpc_plant_settings* settings, double* state, const double* u0, const double* iterate, const double* d,
                                    const double* w) {
    PlantArgs a; unsigned blocks = 0; size_t lds = 0; void* stream = nullptr;
    const pmpc_status st = pmpc_internal_plant_prepare(ctx, Model::NX, Model::NU, Model::NP, Model::ND, P, S, t0, tf, B, dt, settings, state, u0, iterate, d, w,
                                                       &a, &blocks, &lds, &stream);
    if (st != PMPC_OK || blocks == 0) return st;
    if (lds > 64 * 1024) return PMPC_ERR_UNSUPPORTED_SIZE;   // (a model of some 40 states: beyond the static LDS window)
    hipLaunchKernelGGL(plant_kernel<Model>, dim3(blocks), dim3(PLANT_LANES), lds, (hipStream_t)stream, model, a);
    return hipGetLastError() == hipSuccess ? PMPC_OK : PMPC_ERR_HIP;
}

}  // namespace pmpc
