// The K-slice plan of a weight-gradient launch, shared by the fp32 launcher (conv_wgrad.hip: wgrad_launch) and the bf16 one
// (conv_wgrad_bf16.hip: wgrad_bf16_fill); what the kernels make of a plan is conv_wgrad_geom.h.  Host arithmetic only, no HIP:
// tests/test_wgrad_plan_host.py compiles it with g++ and holds it to the plans recorded for tests/wgrad_cases.py and wgrad_bf16_cases.py.
#pragma once
#include <stdint.h>

// When the tiles of a K slice are kept on one XCD (wgrad_place).  Each engine's rule is its own measurement:
//   WGRAD_XCD_FP32: a win (+4..10 %) when a slice has many tiles to share the slabs (>= 16: the 256-channel 3x3 layers), a loss for the
//       few-tile shapes.  tiles >= 16 && splits > 8 && splits + 7 <= max_splits, decided BEFORE the 2 GiB loop with the slices rounded
//       up to 8 (whole slices per XCD: equal shares for the 8); dropped when the loop has to double.
//   WGRAD_XCD_BF16: tiles >= 4 && splits >= 8 of the FINAL slice count (without it: L2 hit rate 39 %, 5.5x the algorithmic bytes
//       fetched, profiles/r02_pmc_conv_bf16.txt).  pad8 (grouped launches): a problem in the plain order rounds its range of the grid
//       up to 8 workgroups, so that every problem's range starts at a multiple of 8 (surplus ids: slice >= splits).
enum WgradXcdPolicy { WGRAD_XCD_FP32, WGRAD_XCD_BF16 };

struct WgradPlanIn {
    int64_t pixels;              // K extent: N * Ho * Wo
    int tiles, target_wgs;       // output tiles (all batch entries); workgroups the launch should bring to the grid
    int wk, ldy, elem_bytes;     // pixels per K-step the slice length is a multiple of; dY row length in elements; bytes per element
    int64_t HoWo, img_bytes;     // output pixels and input bytes of one image
    WgradXcdPolicy policy;
    bool xcd_enabled, pad8;      // WGRAD_XCD_BF16 only: RN_WGRAD_BF16_XCD, and pad8 above
};
struct WgradPlan {
    int64_t per_split;           // pixels per K slice (a multiple of wk)
    int splits, xcd_map;
    int64_t grid;                // workgroups
};

// false: refused (a single image of more than 2 GiB).
static inline bool wgrad_plan(const WgradPlanIn &in, WgradPlan &out) {
    // enough K slices for the target, each at least 16 K-steps long
    int64_t splits = (in.target_wgs + in.tiles - 1) / in.tiles;
    const int64_t max_splits = (in.pixels + 16 * in.wk - 1) / (16 * in.wk);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    int xcd_map = 0;
    if (in.policy == WGRAD_XCD_FP32) {
        xcd_map = in.tiles >= 16 && splits > 8 && splits + 7 <= max_splits;
        if (xcd_map) splits = (splits + 7) / 8 * 8;
    }
    // Buffer-load addressing (see the kernels): the dY bytes of one K slice and the span of input images a slice can touch must each
    // stay below 2 GiB; more slices make both smaller.
    int64_t per_split;
    for (;;) {
        per_split = ((in.pixels + splits - 1) / splits + in.wk - 1) / in.wk * in.wk;
        const int64_t span_imgs = (per_split + in.HoWo - 2) / in.HoWo + 1;
        if ((per_split + in.wk) * in.ldy * in.elem_bytes <= 0x7FFFFFFF && span_imgs * in.img_bytes <= 0x7FFFFFFF) break;
        if (per_split <= in.wk || splits >= 65535) return false;
        splits = splits * 2 > 65535 ? 65535 : splits * 2;
        xcd_map = 0;
    }
    splits = (in.pixels + per_split - 1) / per_split;
    if (in.policy == WGRAD_XCD_BF16) xcd_map = in.xcd_enabled && in.tiles >= 4 && splits >= 8;
    int64_t grid = in.tiles * (xcd_map ? (splits + 7) / 8 * 8 : splits);
    if (in.policy == WGRAD_XCD_BF16 && in.pad8 && !xcd_map) grid = (grid + 7) / 8 * 8;
    out.per_split = per_split;
    out.splits = (int)splits;
    out.xcd_map = xcd_map;
    out.grid = grid;
    return true;
}
