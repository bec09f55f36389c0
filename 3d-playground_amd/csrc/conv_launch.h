// Launch plumbing shared by the implicit-GEMM convolution files (conv_igemm*.hip, conv_bf16*.hip, conv_fp8*.hip): how a workgroup of a
// grouped launch finds its problem, and what the host-side launchers check before they launch.  No kernel code: the tiles, K loops and
// epilogues stay in their own files.  tests/test_conv_launch_host.py pins what these checks refuse and which tile the launchers pick.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ device side: grouped launches
// Which problem of the group owns this tile: a wave-uniform compare chain over the by-value table (tile_end = running tile counts).
__device__ __forceinline__ int rn_group_index(const rn_conv_group &g, const int tile) {
    int p = 0;
#pragma unroll
    for (int i = 0; i < RN_MAX_GROUP - 1; ++i) p += (i + 1 < g.n && tile >= g.tile_end[i]) ? 1 : 0;
    return p;
}
// The kernels with 256-thread tiles then select that problem's descriptor and pointers with STATIC indices into the table (a dynamic
// index would put the by-value kernel argument into scratch memory) -- in place, as an unrolled `if (p == i) { d = g.d[i]; ... }` chain:
// behind a function the compiler selects ADDRESSES in the kernel-argument segment and loads afterwards, and the different scalar
// register pressure re-allocates the whole kernel, K loop included (profiles/conv_launch_refactor_isa.txt).  The phased kernels index
// dynamically, with the index made uniform first: conv_bf16_p8.hip, conv_fp8_p8.hip.

// ------------------------------------------------------------------------------------------------ host side
// Tiles of rows x cols outputs that cover the problem's [N*Ho*Wo][Cout] result.
static inline int64_t rn_conv_tiles(const rn_conv_desc *d, int rows, int cols) {
    const int64_t M = (int64_t)d->N * d->Ho * d->Wo;
    return ((M + rows - 1) / rows) * ((d->Cout + cols - 1) / cols);
}

// The result (and a same-geometry addend) is the plain [N*Ho*Wo][Cout] matrix: the kernels' DENSE / !GENERAL instances skip the output map.
static inline bool rn_conv_dense(const rn_conv_desc *d) {
    return d->os == 1 && d->oo_h == 0 && d->oo_w == 0 && d->Hy == d->Ho && d->Wy == d->Wo &&
           d->y_batch_stride == (int64_t)d->Ho * d->Wo * d->Cout && d->add_mode != 2 &&
           (d->add_mode == 0 || d->add_batch_stride == d->y_batch_stride);
}

// The descriptor rules every form shares.  What differs comes in: elem_bytes of an activation / weight element (a 16-byte chunk must
// not straddle filter taps, so Cin counts whole chunks), tile_rows = the row span of the form's largest tile, k_pad = the multiple the
// packed weight rows are padded to.  Operands are read through 32-bit buffer offsets: the images one tile can touch (which bounds a
// single image too) and the packed weights stay below 2 GiB each, N*Ho*Wo below 2^31.
static inline int rn_check_desc_core(const rn_conv_desc *d, int elem_bytes, int tile_rows, int k_pad) {
    if (d->N <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Cout <= 0) return RN_EINVAL;
    const int chunk = 16 / elem_bytes;
    if (d->Cin < chunk || (d->Cin & (chunk - 1))) return RN_EINVAL;
    const int64_t image = (int64_t)d->Hi * d->Wi * d->Cin, HoWo = (int64_t)d->Ho * d->Wo, span = (tile_rows - 1) / HoWo + 2;
    if (d->x_batch_stride < 0 || ((span - 1) * d->x_batch_stride + image) * elem_bytes > 0x7fffffffLL) return RN_EINVAL;
    const int64_t Kpad = ((int64_t)d->kh * d->kw * d->Cin + k_pad - 1) / k_pad * k_pad;
    if (d->Cout * Kpad * elem_bytes > 0x7fffffffLL || (int64_t)d->N * HoWo > 0x7fffffffLL) return RN_EINVAL;
    if (d->kh <= 0 || d->kw <= 0 || d->div_shift < 0 || d->div_shift > 2) return RN_EINVAL;
    if (d->add_mode < 0 || d->add_mode > 2 || d->act < 0 || d->act > 2) return RN_EINVAL;
    if (d->os < 1 || d->oo_h < 0 || d->oo_w < 0) return RN_EINVAL;
    if ((d->Ho - 1) * d->os + d->oo_h >= d->Hy || (d->Wo - 1) * d->os + d->oo_w >= d->Wy) return RN_EINVAL;
    if (d->os != 1 && d->add_mode == 2) return RN_EINVAL;
    return RN_OK;
}
// The forms with a mask operand (fp32, bf16): its modes, and the sign bits -- read (mask_mode | RN_MASK_BITS) or written (sign_out) --
// which live at element offset >> 5: whole words per pixel and per image.
static inline int rn_check_desc_mask(const rn_conv_desc *d) {
    if (d->mask_mode < 0 || (d->mask_mode & ~(3 | RN_MASK_BITS)) || (d->mask_mode & 3) == 3 || d->mask_mode == RN_MASK_BITS) return RN_EINVAL;
    if (((d->mask_mode & RN_MASK_BITS) || d->sign_out != nullptr) && ((d->Cout & 31) || (d->y_batch_stride & 31))) return RN_EINVAL;
    return RN_OK;
}

// The report of rn_conv_igemm_plan / rn_conv_igemm_grouped_plan (include/retinanet_mi355x.h has the words' meaning).  The fp32 launchers
// carry an `int32_t *plan` down to the statement that launches: with a plan they fill it there, from the very template arguments the launch
// would instantiate, and return before the launch -- one set of rules, asked or run.
enum { RN_PLAN_FAMILY, RN_PLAN_ROWS, RN_PLAN_COLS, RN_PLAN_WAVES, RN_PLAN_GENERAL, RN_PLAN_RELU, RN_PLAN_RAW, RN_PLAN_SPLIT, RN_PLAN_TERMS,
       RN_PLAN_STAGED, RN_PLAN_GRID, RN_PLAN_SLICES, RN_PLAN_USED, RN_PLAN_STEPS, RN_PLAN_FINISH, RN_PLAN_FORM };
enum { RN_PLAN_FAMILY_TILE, RN_PLAN_FAMILY_SPLIT, RN_PLAN_FAMILY_MF16, RN_PLAN_FAMILY_SPLITK };
enum { RN_PLAN_FORM_SINGLE, RN_PLAN_FORM_GROUPED, RN_PLAN_FORM_LIST };
static inline int rn_plan_fill(int32_t *plan, int family, int rows, int cols, int waves, bool general, bool relu, bool raw, int split,
                               int terms, bool staged, unsigned grid, int form) {
    for (int i = 0; i < RN_IGEMM_PLAN_WORDS; ++i) plan[i] = 0;
    plan[RN_PLAN_FAMILY] = family; plan[RN_PLAN_ROWS] = rows; plan[RN_PLAN_COLS] = cols; plan[RN_PLAN_WAVES] = waves;
    plan[RN_PLAN_GENERAL] = general; plan[RN_PLAN_RELU] = relu; plan[RN_PLAN_RAW] = raw; plan[RN_PLAN_SPLIT] = split;
    plan[RN_PLAN_TERMS] = terms; plan[RN_PLAN_STAGED] = staged; plan[RN_PLAN_GRID] = (int32_t)grid; plan[RN_PLAN_FINISH] = -1;
    plan[RN_PLAN_FORM] = form;
    return RN_OK;
}

// A grouped launch: 1 .. RN_MAX_GROUP problems, each passing the form's own check(desc, index) (RN_OK or an error), all with the first
// one's channels and filter, and the caller's tile_end = the running count of rows x cols tiles.  *tiles receives the grid size.
template <class Check>
static inline int rn_check_group(const rn_conv_group *g, int rows, int cols, Check check, int *tiles) {
    if (g->n < 1 || g->n > RN_MAX_GROUP) return RN_EINVAL;
    const rn_conv_desc &d0 = g->d[0];
    int prev = 0;
    for (int i = 0; i < g->n; ++i) {
        const rn_conv_desc &d = g->d[i];
        const int rc = check(d, i);
        if (rc) return rc;
        if (d.Cin != d0.Cin || d.Cout != d0.Cout || d.kh != d0.kh || d.kw != d0.kw) return RN_EINVAL;
        if (g->tile_end[i] - prev != rn_conv_tiles(&d, rows, cols)) return RN_EINVAL;
        prev = g->tile_end[i];
    }
    *tiles = prev;
    return RN_OK;
}
