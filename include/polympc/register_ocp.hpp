// polympc_amd — register a user-defined OCP for the GPU.
//
// The reference lets a user define an OCP as a C++ class with templated dynamics_impl<T> / lagrange_term_impl<T> /
// mayer_term_impl<T> / inequality_constraints_impl<T> (continuous_ocp.hpp:191-288; example
// tests/control/mpc_wrapper_test.cpp:37-80) and differentiates it with nested AutoDiffScalar. Here the same class body
// is compiled by hipcc: the templates are instantiated with pmpc::Dual (device forward-mode AD) inside the fused SQP
// kernel. Write the class against pmpc::cref<T> / pmpc::vref<T> views (element access x(i), as with Eigen::Ref), mark
// the four functions __device__, give it `enum { NX, NU, NP, ND, NG }`, and in ONE .hip translation unit:
//
//     #include <polympc/register_ocp.hpp>
//     struct MyOCP { enum { NX = 2, NU = 1, NP = 0, ND = 0, NG = 0 }; ... };
//     PMPC_REGISTER_OCP(MyOCP)
//
// compiled with:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared my_ocp.hip
//                       -I<repo>/include -L<repo>/polympc_amd -lpolympc_amd -o libmy_ocp.so
// This emits the C symbols pmpc_user_sqp_dev_MyOCP (device buffers, type pmpc_sqp_dev_fn), pmpc_user_dims_MyOCP and pmpc_user_plant_dev_MyOCP
// (type pmpc_plant_dev_fn: one control period of x' = dynamics_impl integrated on the device, the plant of a closed loop — pmpc_plant.hpp).
// and pmpc_user_lin_dev_MyOCP (type pmpc_lin_dev_fn: the collocation assembly with the exact Lagrangian Hessian at given points, the linearisation of
// pmpc_ocp_linearise_batch_user and of the KKT refinement pmpc_sqp_refine_batch_user / pmpc_mpc_batch_set_lineariser).
// Host code (any C++ compiler) then uses polympc::Solver<...> from <polympc/polympc.hpp> with POLYMPC_USE_REGISTERED_OCP.
#pragma once
#include "../polympc_amd.h"
#include "../../polympc_amd/csrc/pmpc_launch.hpp"
#include "../../polympc_amd/csrc/pmpc_plant.hpp"

#define PMPC_REGISTER_OCP(Name)                                                                                                  \
    extern "C" pmpc_status pmpc_user_sqp_dev_##Name(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf,   \
                                                    int B, const double* x_guess, const double* lam_guess, const double* d,     \
                                                    const double* lbx, const double* ubx, const double* lbg, const double* ubg, \
                                                    const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x,         \
                                                    double* lam, pmpc_sqp_info* info) {                                         \
        return pmpc::sqp_launch_dev<Name>(ctx, *static_cast<const Name*>(model), P, S, t0, tf, B, x_guess, lam_guess, d, lbx,   \
                                          ubx, lbg, ubg, ss, qs, x, lam, info);                                                 \
    }                                                                                                                            \
    extern "C" void pmpc_user_dims_##Name(int* nx, int* nu, int* np, int* nd, int* ng) {                                        \
        *nx = Name::NX; *nu = Name::NU; *np = Name::NP; *nd = Name::ND; *ng = Name::NG;                                          \
    }                                                                                                                            \
    extern "C" pmpc_status pmpc_user_plant_dev_##Name(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf,  \
                                                      int B, double dt, const pmpc_plant_settings* settings, double* state,     \
                                                      const double* u0, const double* iterate, const double* d,                 \
                                                      const double* w) {                                                        \
        if (!model) return PMPC_ERR_INVALID_ARGUMENT;                                                                            \
        return pmpc::plant_launch_dev<Name>(ctx, *static_cast<const Name*>(model), P, S, t0, tf, B, dt, settings, state, u0,     \
                                            iterate, d, w);                                                                      \
    }                                                                                                                            \
    extern "C" pmpc_status pmpc_user_lin_dev_##Name(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf,    \
                                                    int B, const double* var, const double* d, const double* lam, double* cost, \
                                                    double* constr, double* jac, double* cost_grad, double* lag_grad,           \
                                                    double* lag_hess) {                                                         \
        if (!model) return PMPC_ERR_INVALID_ARGUMENT;                                                                            \
        return pmpc::linearise_launch_dev<Name>(ctx, *static_cast<const Name*>(model), P, S, t0, tf, B, var, d, lam, cost,       \
                                                constr, jac, cost_grad, lag_grad, lag_hess);                                     \
    }
