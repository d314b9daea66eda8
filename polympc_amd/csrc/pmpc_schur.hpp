// polympc_amd — block-structured specialisations of the fused SQP kernel (pmpc_qp_schur.hpp) per built-in model: one translation unit per model
// (pmpc_schur_*.hip), compiled in parallel to the dense kernels. Grids: the BASELINE configurations and the reference's own test grids.
#pragma once
#include "pmpc_context.hpp"
#include "pmpc_models.hpp"
#include "pmpc_launch.hpp"

#define PMPC_SCHUR_ARGS pmpc_context* ctx, const pmpc::SqpArgs<MODEL>& a, pmpc::SqpPlan<MODEL>& p
#define PMPC_SCHUR_PLAN(PP, SS) \
    if (pmpc::plan_schur<MODEL, PP, SS>(ctx, a, p)) return true;
