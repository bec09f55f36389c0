// Host program around the weight gradients' slice planner (3d-playground_amd/csrc/conv_wgrad_plan.h, the header both launchers
// compile).  Reads one problem per line -- pixels tiles target_wgs wk ldy elem_bytes HoWo img_bytes policy xcd_enabled pad8 -- and
// prints its plan: per_split splits xcd_map grid, or "refused".  Built and run by tests/test_wgrad_plan_host.py (g++, no GPU).
#include <cstdio>

#include "conv_wgrad_plan.h"

int main() {
    long long pixels, HoWo, img_bytes;
    int tiles, target, wk, ldy, elem, policy, xcd_enabled, pad8;
    while (std::scanf("%lld %d %d %d %d %d %lld %lld %d %d %d", &pixels, &tiles, &target, &wk, &ldy, &elem, &HoWo, &img_bytes, &policy,
                      &xcd_enabled, &pad8) == 11) {
        const WgradPlanIn in = {pixels, tiles, target, wk, ldy, elem, HoWo, img_bytes, policy ? WGRAD_XCD_BF16 : WGRAD_XCD_FP32,
                                xcd_enabled != 0, pad8 != 0};
        WgradPlan pl;
        if (!wgrad_plan(in, pl)) std::printf("refused\n");
        else std::printf("%lld %d %d %lld\n", (long long)pl.per_split, pl.splits, pl.xcd_map, (long long)pl.grid);
    }
    return 0;
}
