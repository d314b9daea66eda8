// Prints the dynamic LDS bytes the launcher requests (plan_reg, pmpc_launch.hpp) for every register grid of the built-in models: one line
// "model P S nodes rows full full_hooks condensed" per grid (0: the launcher has no such request). Host code only; compiled and run by
// tests/test_static_layout_cpu.py, which compares the table with the one recorded before the static layout (tests/golden/lds_totals_r09.txt).
#include <cstdio>
#include "../../polympc_amd/csrc/pmpc_launch.hpp"
using namespace pmpc;

template <class Model, int NNODES> void grid(const char* name, int P, int S) {
    constexpr int NN_ = (Model::NX + Model::NU) * NNODES + Model::NP, MM_ = (Model::NX + Model::NG) * NNODES;
    if constexpr (NN_ + MM_ <= 128) {
        constexpr SqpLdsLayout layout = NN_ + MM_ <= WAVE ? SqpLdsLayout::Reg1 : (NN_ + MM_ <= 112 ? SqpLdsLayout::Reg2 : SqpLdsLayout::Reg2LdsTiles);
        size_t cond = 0;
        if constexpr (COND_REG_OK<Model, NN_, MM_>::value) {
            if constexpr (NN_ <= WAVE) cond = sqp_kernel_lds_bytes<Model>(P, S, SqpLdsLayout::Cond1);
            else cond = sqp_kernel_lds_bytes<Model>(P, S, SqpLdsLayout::Cond2, 0, false, (size_t)cond_qp_staging<NN_, MM_, NNODES>());
        }
        std::printf("%s %d %d %d %d %zu %zu %zu\n", name, P, S, NNODES, NN_ + MM_, sqp_kernel_lds_bytes<Model>(P, S, layout, 0, false),
                    sqp_kernel_lds_bytes<Model>(P, S, layout, 0, true), cond);
    }
}
template <class Model, int NNODES> void nodes(const char* name) {
    for (int P = 1; P <= MAX_P; ++P)
        for (int S = 1; S <= 15; ++S)
            if (P * S + 1 == NNODES) grid<Model, NNODES>(name, P, S);
    if constexpr (NNODES < 16) nodes<Model, NNODES + 1>(name);
}
int main() {
    nodes<RobotOCP, 3>("robot"); nodes<CstrOCP, 3>("cstr"); nodes<ParkingOCP, 3>("parking"); nodes<ParkingNGOCP, 3>("parking_ng"); nodes<RobotNGOCP, 3>("robot_ng");
    return 0;
}
