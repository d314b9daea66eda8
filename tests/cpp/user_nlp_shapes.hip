// The size-range NLPs of oracle/nlp_shapes.hpp registered for the GPU as a user would register them (PMPC_REGISTER_NLP), from the same
// bodies the CPU checker compiles, plus test-only C entry points around pmpc::nlp_linearise_dev<Def>: the product exposes linearisation
// for its built-in problems only. Built by tests/cpp/nlp.mk; used by tests/test_gpu_nlp_shapes.py and tests/test_nlp_cpu.py.
#include <polympc/register_nlp.hpp>
#include "../../oracle/nlp_shapes.hpp"

// the device problem concept (pmpc_nlp.hpp) over a shared body
template <class Body>
struct DeviceShape {
    enum { NX = Body::NX, NE = Body::NE, NI = Body::NI, NP = Body::NP };
    template <class T> __device__ void cost_impl(pmpc::cref<T> x, pmpc::cref<double> p, T& cost) const { Body::cost(x, p, cost); }
    template <class T> __device__ void equality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ce) const {
        Body::template eq<T>(x, p, ce);
    }
    template <class T> __device__ void inequality_constraints_impl(pmpc::cref<T> x, pmpc::cref<double> p, pmpc::vref<T> ci) const {
        Body::template ineq<T>(x, p, ci);
    }
};

// host buffers in and out (B instances; lam: m + nx per instance; d: NP per instance, may be null when NP = 0)
template <class Def>
static pmpc_status linearise_host(pmpc_context* ctx, int B, const double* x, const double* lam, const double* d, double* cost, double* constr,
                                  double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    const size_t n = Def::NX, m = Def::NE + Def::NI, np = Def::NP;
    const size_t sz[9] = {B * n, B * (m + n), B * (np ? np : 1), (size_t)B, B * (m ? m : 1), B * (m ? m : 1) * n, B * n, B * n, B * n * n};
    double* buf[9] = {};
    pmpc_status st = PMPC_OK;
    for (int i = 0; i < 9 && st == PMPC_OK; ++i)
        if (hipMalloc((void**)&buf[i], sz[i] * sizeof(double)) != hipSuccess) st = PMPC_ERR_HIP;
    if (st == PMPC_OK && (hipMemcpy(buf[0], x, sz[0] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(buf[1], lam, sz[1] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                          (np && hipMemcpy(buf[2], d, sz[2] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)))
        st = PMPC_ERR_HIP;
    if (st == PMPC_OK)
        st = pmpc::nlp_linearise_dev(ctx, Def{}, B, buf[0], buf[1], np ? buf[2] : nullptr, buf[3], m ? buf[4] : nullptr, m ? buf[5] : nullptr,
                                     buf[6], buf[7], buf[8]);
    if (st == PMPC_OK && hipDeviceSynchronize() != hipSuccess) st = PMPC_ERR_HIP;
    double* out[6] = {cost, constr, jac, cost_grad, lag_grad, lag_hess};
    for (int i = 0; i < 6 && st == PMPC_OK; ++i)
        if ((i != 1 && i != 2) || m)
            if (hipMemcpy(out[i], buf[3 + i], sz[3 + i] * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) st = PMPC_ERR_HIP;
    for (int i = 0; i < 9; ++i) if (buf[i]) (void)hipFree(buf[i]);
    return st;
}

#define SHAPE(Name)                                                                                                                   \
    using Name = DeviceShape<nlp_shapes::Name>;                                                                                       \
    PMPC_REGISTER_NLP(Name)                                                                                                           \
    extern "C" pmpc_status pmpc_test_nlp_linearise_##Name(pmpc_context* ctx, int B, const double* x, const double* lam, const double* d, \
                                                           double* cost, double* constr, double* jac, double* cost_grad,              \
                                                           double* lag_grad, double* lag_hess) {                                      \
        return linearise_host<Name>(ctx, B, x, lam, d, cost, constr, jac, cost_grad, lag_grad, lag_hess);                            \
    }

SHAPE(ChainRosen9)
SHAPE(Sphere12)
SHAPE(Cuts8)
SHAPE(Wave64)
SHAPE(Wide60)
SHAPE(Unc64)
SHAPE(Param70)
