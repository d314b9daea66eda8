// polympc_amd — register a user-defined NLP for the GPU.
//
// The reference lets a user define an NLP as a C++ class with templated cost_impl<T> / equality_constraints_impl<T> /
// inequality_constraints_impl<T> (src/solvers/nlproblem.hpp; examples tests/solvers/sqp/sqp_test_autodiff.cpp) and differentiates it
// with AutoDiffScalar. Here the same class body is compiled by hipcc: the templates are instantiated with pmpc::Dual (device forward-mode
// AD) inside the batched SQP kernel. Write the class against pmpc::cref<T> / pmpc::vref<T> views (element access x(i), as with
// Eigen::Ref; the static parameters arrive as pmpc::cref<double> p), mark the three functions __device__, give it
// `enum { NX, NE, NI, NP }`, and in ONE .hip translation unit:
//
//     #include <polympc/register_nlp.hpp>
//     struct MyNLP { enum { NX = 4, NE = 1, NI = 1, NP = 0 }; ... };
//     PMPC_REGISTER_NLP(MyNLP)
//
// compiled with:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared my_nlp.hip
//                       -I<repo>/include -L<repo>/polympc_amd -lpolympc_amd -o libmy_nlp.so
// This emits the C symbols pmpc_user_nlp_sqp_dev_MyNLP (device buffers, type pmpc_nlp_dev_fn) and pmpc_user_nlp_dims_MyNLP.
// Host code (any C++ compiler) then uses polympc::NlpSolver<...> from <polympc/polympc.hpp> with POLYMPC_USE_REGISTERED_NLP.
#pragma once
#include "../polympc_amd.h"
#include "../../polympc_amd/csrc/pmpc_nlp.hpp"

#define PMPC_REGISTER_NLP(Name)                                                                                                    \
    extern "C" pmpc_status pmpc_user_nlp_sqp_dev_##Name(pmpc_context* ctx, const void* model, int B, const double* x_guess,      \
                                                        const double* lam_guess, const double* d, const double* lbx,              \
                                                        const double* ubx, const double* lbg, const double* ubg,                  \
                                                        const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x,       \
                                                        double* lam, pmpc_sqp_info* info) {                                       \
        if (!model) return PMPC_ERR_INVALID_ARGUMENT;                                                                              \
        return pmpc::nlp_launch_dev<Name>(ctx, *static_cast<const Name*>(model), B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, \
                                          qs, x, lam, info);                                                                       \
    }                                                                                                                              \
    extern "C" void pmpc_user_nlp_dims_##Name(int* nx, int* ne, int* ni, int* np) {                                                \
        *nx = Name::NX; *ne = Name::NE; *ni = Name::NI; *np = Name::NP;                                                            \
    }
