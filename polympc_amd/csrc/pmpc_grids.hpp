// polympc_amd — register-resident specialisations of the fused SQP kernel for further node counts of the built-in models: 3, 4, 6, 8, 9, 10, 12, 13 and 14 nodes — one KKT row
// per lane (pmpc_qp_reg.hpp) where n + m <= 64, two rows per lane (pmpc_qp_reg2.hpp) where 64 < n + m <= 112, nothing where the system is larger. The 5-, 7- and
// 11-node grids are part of every model's own translation unit (pmpc_launch.hpp); these compile in parallel to them, one translation unit per model
// (pmpc_grids_*.hip), without the phase-timer and block-BFGS variants (such requests take the LDS-resident kernel).
#pragma once
#include "pmpc_context.hpp"
#include "pmpc_models.hpp"
#include "pmpc_launch.hpp"

namespace pmpc {

template <class Model>
bool plan_extra_grids(pmpc_context* ctx, const SqpArgs<Model>& a, SqpPlan<Model>& p) {
    return plan_reg<Model, 3, true>(ctx, a, p) || plan_reg<Model, 4, true>(ctx, a, p) || plan_reg<Model, 6, true>(ctx, a, p) ||
           plan_reg<Model, 8, true>(ctx, a, p) || plan_reg<Model, 9, true>(ctx, a, p) || plan_reg<Model, 10, true>(ctx, a, p) ||
           plan_reg<Model, 12, true>(ctx, a, p) || plan_reg<Model, 13, true>(ctx, a, p) || plan_reg<Model, 14, true>(ctx, a, p) ||
           plan_reg<Model, 15, true>(ctx, a, p) || plan_reg<Model, 16, true>(ctx, a, p);   // 15, 16: 113..128 rows where the model fits them (robot: 15 and 16 nodes — the reference's mpc_wrapper_test grid; CSTR: 12 above)
}

}  // namespace pmpc

#define PMPC_INSTANTIATE_GRIDS(MODEL) \
    template bool pmpc::plan_extra_grids<MODEL>(pmpc_context*, const pmpc::SqpArgs<MODEL>&, pmpc::SqpPlan<MODEL>&);
