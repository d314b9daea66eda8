// Direct probes of the device AD scalar (pmpc_ad.hpp) and of pmpc::detmath through it, plus one NLP that uses every function no built-in
// model uses, registered as a user registers one. Every probe body is ONE __host__ __device__ template, evaluated by a kernel (one point per
// lane, full workgroups of 64, bounds check on the tail) and by a host loop; `on_device` selects which. Nothing from oracle/ is included.
// Built by tests/cpp/Makefile with the product's flags; used by tests/test_ad_probe_cpu.py, tests/test_gpu_ad_probe.py and
// tests/test_gpu_nlp_exact.py.
#include <polympc/register_nlp.hpp>
#include "../../polympc_amd/csrc/pmpc_ad.hpp"
#include "../../polympc_amd/csrc/pmpc_models.hpp"

namespace probe {

using pmpc::cref;
using pmpc::Dual;
using pmpc::Value;
using pmpc::vref;

// ------------------------------------------------------------------------------------------------ maths
enum { FN_SIN = 0, FN_COS, FN_SINCOS_S, FN_SINCOS_C, FN_EXP, FN_COUNT };

__host__ __device__ inline double math_eval(int fn, double x) {
    double s, c;
    switch (fn) {
        case FN_SIN: return pmpc::m_sin(x);
        case FN_COS: return pmpc::m_cos(x);
        case FN_SINCOS_S: pmpc::m_sincos(x, s, c); return s;
        case FN_SINCOS_C: pmpc::m_sincos(x, s, c); return c;
        default: return pmpc::m_exp(x);
    }
}

__global__ void math_kernel(int fn, int n, const double* x, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = math_eval(fn, x[i]);
}

// ------------------------------------------------------------------------------------------------ AD expressions of (a, b, c) = (x(0), x(1), x(2))
enum { EX_ADD = 0, EX_SUB, EX_NEG, EX_MUL, EX_DIV, EX_CMUL, EX_SIN, EX_COS, EX_SINCOS_S, EX_SINCOS_C, EX_EXP, EX_SQRT, EX_ARRHENIUS, EX_NORM2,
       EX_ROBOT, EX_INVSQ, EX_MIXED, EX_COUNT };

template <class T>
__host__ __device__ T expr_eval(int id, cref<T> x) {
    T s, c;
    switch (id) {
        case EX_ADD: return x(0) + x(1);
        case EX_SUB: return x(0) - x(1);
        case EX_NEG: return -x(0);
        case EX_MUL: return x(0) * x(1);
        case EX_DIV: return x(0) / x(1);
        case EX_CMUL: return T(2.5) * x(0);
        case EX_SIN: return sin(x(0));
        case EX_COS: return cos(x(0));
        case EX_SINCOS_S: sincos(x(0), s, c); return s;
        case EX_SINCOS_C: sincos(x(0), s, c); return c;
        case EX_EXP: return exp(x(0));
        case EX_SQRT: return sqrt(x(0));
        case EX_ARRHENIUS: return exp(T(-9758.3) / (T(273.15) + x(0)));                 // the CSTR's Arrhenius factor
        case EX_NORM2: return sqrt(x(0) * x(0) + x(1) * x(1));
        case EX_ROBOT: return x(0) * sin(x(1)) * cos(x(2)) / T(2.0);                     // u * sin(x) * cos(y) / d
        case EX_INVSQ: return x(0) / (x(1) * x(1));
        default: return sqrt(x(0)) * exp(-x(1)) / (T(1.0) + x(2) * x(2));               // EX_MIXED
    }
}

enum { MODE_VALUE = 0, MODE_D1, MODE_D2, MODE_SEEDED, MODE_COUNT };
constexpr int NV = 3, NOUT = 13;   // out: value, 3 first derivatives, 9 second derivatives H[r][dir] at 4 + 3 r + dir

__host__ __device__ inline void ad_point(int expr, int mode, const double* in, double* out) {
    for (int k = 0; k < NOUT; ++k) out[k] = 0.0;
    if (mode == MODE_VALUE) {
        out[0] = expr_eval<Value>(expr, pmpc::as_cvalues(in)).v;
    } else if (mode == MODE_D1) {
        using D1 = Dual<double, NV>;
        D1 x[NV];
        for (int i = 0; i < NV; ++i) { x[i] = D1(in[i]); x[i].d[i] = 1.0; }
        const D1 r = expr_eval<D1>(expr, cref<D1>(x));
        out[0] = r.v;
        for (int i = 0; i < NV; ++i) out[1 + i] = r.d[i];
    } else if (mode == MODE_D2) {
        // second-order seeding of the full nested form: outer derivative = unit, inner value's derivative = unit
        using D1 = Dual<double, NV>;
        using D2 = Dual<D1, NV>;
        D2 x[NV];
        for (int i = 0; i < NV; ++i) { D2 t; t.v = D1(in[i]); t.v.d[i] = 1.0; t.d[i] = D1(1.0); x[i] = t; }
        const D2 r = expr_eval<D2>(expr, cref<D2>(x));
        out[0] = r.v.v;
        for (int i = 0; i < NV; ++i) out[1 + i] = r.v.d[i];
        for (int rr = 0; rr < NV; ++rr)
            for (int dir = 0; dir < NV; ++dir) out[4 + NV * rr + dir] = r.d[dir].d[rr];
    } else {
        // the kernels' seeded form: one evaluation per (r, dir), the variables generated where the expression reads them
        using S2 = Dual<Dual<double, 1>, 1>;
        for (int rr = 0; rr < NV; ++rr)
            for (int dir = 0; dir < NV; ++dir) {
                const S2 r = expr_eval<S2>(expr, cref<S2>(in, 0, rr, dir));
                if (rr == 0 && dir == 0) out[0] = r.v.v;
                if (rr == dir) out[1 + rr] = r.v.d[0];
                out[4 + NV * rr + dir] = r.d[0].d[0];
            }
    }
}

__global__ void ad_kernel(int expr, int mode, int n, const double* in, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ad_point(expr, mode, in + (size_t)i * NV, out + (size_t)i * NOUT);
}

// device buffers around one launch: copies `in` up, runs `launch(din, dout)`, copies `out` back; 0 or the failing hipError_t
template <class Launch>
static int on_gpu(const double* in, size_t nin, double* out, size_t nout, Launch launch) {
    double *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, nin * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, nout * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(din, in, nin * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch(din, dout); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

}  // namespace probe

extern "C" int pmpc_probe_math(int fn, int on_device, int n, const double* x, double* out) {
    if (fn < 0 || fn >= probe::FN_COUNT || n <= 0 || !x || !out) return -1;
    if (!on_device) {
        for (int i = 0; i < n; ++i) out[i] = probe::math_eval(fn, x[i]);
        return 0;
    }
    return probe::on_gpu(x, (size_t)n, out, (size_t)n, [&](const double* dx, double* dout) {
        hipLaunchKernelGGL(probe::math_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, fn, n, dx, dout);
    });
}

extern "C" int pmpc_probe_ad(int expr, int mode, int on_device, int n, const double* in, double* out) {
    if (expr < 0 || expr >= probe::EX_COUNT || mode < 0 || mode >= probe::MODE_COUNT || n <= 0 || !in || !out) return -1;
    if (!on_device) {
        for (int i = 0; i < n; ++i) probe::ad_point(expr, mode, in + (size_t)i * probe::NV, out + (size_t)i * probe::NOUT);
        return 0;
    }
    return probe::on_gpu(in, (size_t)n * probe::NV, out, (size_t)n * probe::NOUT, [&](const double* din, double* dout) {
        hipLaunchKernelGGL(probe::ad_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, expr, mode, n, din, dout);
    });
}

// ------------------------------------------------------------------------------------------------ the production linearisation kernel on sqrt / exp / sincos / division
// NX = 5, NE = 2, NI = 1, NP = 2: every function and operator appears in the cost and in a constraint; the static parameters inside a sqrt and an exp.
// tests/nlp_exact_ref.py restates it in sympy.
struct ProbeNlp {
    enum { NX = 5, NE = 2, NI = 1, NP = 2 };
    template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double> p, T& cost) const {
        T s, c;
        sincos(x(2), s, c);
        cost = sqrt(x(0) * x(1) + T(p(0))) * exp(-(T(p(1)) * x(2))) + sin(x(3)) * (x(0) + x(1)) / cos(x(4)) + c / s;
    }
    template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ce) const {
        T s, c;
        sincos(x(1) + x(4), s, c);
        ce(0) = exp(x(0) - x(1)) / sqrt(x(2)) - cos(x(3)) + (-x(4)) * sin(x(0));
        ce(1) = s * x(2) - c / (x(3) + T(p(1)));
    }
    template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ci) const {
        T s, c;
        sincos(x(2), s, c);
        ci(0) = sqrt(x(3) * x(3) + x(4) * x(4) + T(p(0))) * exp(T(p(1)) * x(0)) - sin(x(1)) / x(2) + (-c) * cos(x(0)) * s;
    }
};
PMPC_REGISTER_NLP(ProbeNlp)

// host buffers in and out (B instances; lam: m + nx per instance; d: NP per instance), as tests/cpp/user_nlp_shapes.hip has it
extern "C" pmpc_status pmpc_test_nlp_linearise_ProbeNlp(pmpc_context* ctx, int B, const double* x, const double* lam, const double* d, double* cost,
                                                         double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    using Def = ProbeNlp;
    if (B <= 0 || !x || !lam || !d) return PMPC_ERR_INVALID_ARGUMENT;
    const size_t n = Def::NX, m = Def::NE + Def::NI, np = Def::NP;
    const size_t sz[9] = {B * n, B * (m + n), B * np, (size_t)B, B * m, B * m * n, B * n, B * n, B * n * n};
    double* buf[9] = {};
    pmpc_status st = PMPC_OK;
    for (int i = 0; i < 9 && st == PMPC_OK; ++i)
        if (hipMalloc((void**)&buf[i], sz[i] * sizeof(double)) != hipSuccess) st = PMPC_ERR_HIP;
    if (st == PMPC_OK && (hipMemcpy(buf[0], x, sz[0] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(buf[1], lam, sz[1] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(buf[2], d, sz[2] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
        st = PMPC_ERR_HIP;
    if (st == PMPC_OK) st = pmpc::nlp_linearise_dev(ctx, Def{}, B, buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], buf[6], buf[7], buf[8]);
    if (st == PMPC_OK && hipDeviceSynchronize() != hipSuccess) st = PMPC_ERR_HIP;
    double* out[6] = {cost, constr, jac, cost_grad, lag_grad, lag_hess};
    for (int i = 0; i < 6 && st == PMPC_OK; ++i)
        if (hipMemcpy(out[i], buf[3 + i], sz[3 + i] * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) st = PMPC_ERR_HIP;
    for (int i = 0; i < 9; ++i) if (buf[i]) (void)hipFree(buf[i]);
    return st;
}
