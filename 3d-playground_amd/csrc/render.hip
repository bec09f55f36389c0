// MC_Crop_Tracker.plot (MC3D_crop_tracker.py:733-917) and Homography.plot_boxes (homography.py:670-714) without cv2: the
// output frames of the tracker, drawn on the device from what is already there.
//
// The reference copies every frame to float64, draws with cv2, blends two more full copies and tiles the cameras into a
// float64 canvas, on the host.  Here every primitive ORs one bit into a mask plane uint16 [n_cam,H,W] (include/
// retinanet_mi355x.h: RN_RENDER_*), and ONE pass reads the frames the detector already has (12 B per pixel) and the mask (2 B)
// and writes the uint8 mosaic (3 B).  Every layer has one colour and the layer order is fixed in the compose pass, so a
// pixel's mask decides its result whatever order the primitives arrive in: the picture is bit-identical from run to run.
//
//   rn_render_edges    one workgroup per box edge; exact integer coverage rule (below), no division in the test
//   rn_render_rects    one workgroup per rectangle, one atomic per 32-bit mask word (two pixels)
//   rn_render_text     one workgroup per run of bytes, 6x8 cells from a glyph table passed in
//   rn_render_compose  four pixels per lane, 16-byte loads where the row allows them
//
// Atomics: integer atomicOr on the aligned 32-bit word holding pixels 2k and 2k + 1 of the flattened plane (the plane's buffer
// reaches to a multiple of 4 bytes).  OR commutes, so contention costs time, never bits.
// This file is in the Makefile's EXACT list (no fma contraction): the compose pass rounds once per operation.
#include "common.h"

#define RD_THREADS 256
#define RD_COORD_MIN (-8192)
#define RD_COORD_MAX 8191

__constant__ int rd_edge_a[14] = {0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 6};      // homography.py:679-686, row by row
__constant__ int rd_edge_b[14] = {1, 2, 4, 3, 5, 3, 6, 7, 6, 7, 5, 6, 7, 7};

// int(v) of Python for a finite v inside the coordinate range; false for anything else
__device__ __forceinline__ bool rd_trunc(double v, int &out) {
    if (!(v > (double)RD_COORD_MIN - 1.0 && v < (double)RD_COORD_MAX + 1.0)) return false;        // NaN and inf fail here
    out = (int)v;                                                                                  // toward zero
    return true;
}

// floor(a / b) for b > 0
__device__ __forceinline__ int rd_floordiv(int a, int b) {
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// OR `bits` into pixel p (flattened index over the whole plane) -- p is inside the plane
__device__ __forceinline__ void rd_or_pixel(unsigned *words, int64_t p, unsigned bits) {
    atomicOr(words + (p >> 1), bits << ((unsigned)(p & 1) << 4));
}

// (int(min x), int(max y)) of the eight corners of an anchor box; false when a corner is not finite or out of range
__device__ __forceinline__ bool rd_anchor(const double *__restrict__ anchors, int64_t n_anchor, int a, int &ax, int &ay) {
    if ((int64_t)a >= n_anchor) return false;
    const double *c = anchors + (int64_t)a * 16;
    double mx = c[0], my = c[1];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double x = c[2 * k], y = c[2 * k + 1];
        int t;
        ok = ok && rd_trunc(x, t) && rd_trunc(y, t);
        mx = x < mx ? x : mx;
        my = y > my ? y : my;
    }
    return ok && rd_trunc(mx, ax) && rd_trunc(my, ay);
}

// ---------------------------------------------------------------------------------------------- edges
// Pixel (x, y) is covered when 4 d^2 <= t^2, d the distance to the segment A-B.  With w = P - A, e = B - A: the projection
// falls inside when 0 < w.e < e.e, then d^2 = cross(w, e)^2 / e.e; otherwise d is the distance to the nearer endpoint.
// |coordinates| <= 8192 and pixels < 16384: |w| < 2^15, |e| < 2^14 + 1, cross^2 < 2^60, everything fits int64.
__device__ __forceinline__ bool rd_covered(int x, int y, int ax, int ay, int bx, int by, int64_t tt) {
    const int64_t ex = bx - ax, ey = by - ay, wx = x - ax, wy = y - ay;
    const int64_t len2 = ex * ex + ey * ey, dot = wx * ex + wy * ey;
    if (len2 == 0 || dot <= 0) return 4 * (wx * wx + wy * wy) <= tt;
    if (dot >= len2) {
        const int64_t ux = x - bx, uy = y - by;
        return 4 * (ux * ux + uy * uy) <= tt;
    }
    const int64_t cr = wx * ey - wy * ex;
    return 4 * cr * cr <= tt * len2;
}

// One workgroup per edge.  Rows [ymin - r, ymax + r] of the frame; in row y only points of the segment with a y coordinate in
// [y - r, y + r] can be within r, and x is monotone along the segment, so the candidates of the row lie between the segment's
// x at those two heights, widened by r (and by 1 for the floor): a superset, tested exactly.  Work is flattened over
// (row, word of the widest interval) so that steep and shallow edges both fill the lanes; a lane tests the two pixels of its
// 32-bit word and issues one atomic for both.
__global__ void __launch_bounds__(RD_THREADS) rd_edges_kernel(const double *__restrict__ corners, const int32_t *__restrict__ cam,
                                                              int thickness, unsigned bits, unsigned *__restrict__ words, int n_cam,
                                                              int H, int W) {
    const int64_t box = blockIdx.x / 14;
    const int e = blockIdx.x % 14;
    const int c = cam[box];
    if (c < 0 || c >= n_cam) return;
    const double *pa = corners + box * 16 + 2 * rd_edge_a[e], *pb = corners + box * 16 + 2 * rd_edge_b[e];
    int ax, ay, bx, by;
    if (!rd_trunc(pa[0], ax) || !rd_trunc(pa[1], ay) || !rd_trunc(pb[0], bx) || !rd_trunc(pb[1], by)) return;
    if (ay > by) {                                                   // A is the upper endpoint (the rule is symmetric)
        int t = ax; ax = bx; bx = t;
        t = ay; ay = by; by = t;
    }
    const int r = (thickness + 1) / 2;
    const int64_t tt = (int64_t)thickness * thickness;
    const int dy = by - ay, dx = bx - ax, adx = dx < 0 ? -dx : dx;
    const int y_lo = max(ay - r, 0), y_hi = min(by + r, H - 1);
    const int x_min = min(ax, bx), x_max = max(ax, bx);
    if (y_lo > y_hi || x_max + r < 0 || x_min - r >= W) return;
    // the widest a row's interval can be: the x run over 2r rows of height, + 1 for the floors, + 2r
    const int span = dy == 0 ? adx : min(adx, (int)(((int64_t)adx * (2 * r)) / dy) + 1);
    const int wmax = span + 2 * r + 2;
    const int wpr = wmax / 2 + 2;                                    // 32-bit words (two pixels) a row's interval can touch
    const int64_t items = (int64_t)(y_hi - y_lo + 1) * wpr;
    const int64_t plane = (int64_t)c * H * W;
    for (int64_t it = threadIdx.x; it < items; it += RD_THREADS) {
        const int y = y_lo + (int)(it / wpr), k = (int)(it % wpr);
        int lo, hi;
        if (dy == 0) {
            lo = x_min;
            hi = x_max;
        } else {
            const int ya = min(max(y - r, ay), by), yb = min(max(y + r, ay), by);
            const int fa = ax + rd_floordiv(dx * (ya - ay), dy), fb = ax + rd_floordiv(dx * (yb - ay), dy);
            lo = min(fa, fb);
            hi = max(fa, fb) + 1;
        }
        const int xl = max(lo - r, 0), xh = min(hi + r, W - 1);
        if (xl > xh) continue;
        const int64_t row = plane + (int64_t)y * W, pl = row + xl, ph = row + xh;                 // pixels [pl, ph] of the plane
        const int64_t w = (pl >> 1) + k;
        if (w > (ph >> 1)) continue;
        unsigned v = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t p = 2 * w + h;
            if (p >= pl && p <= ph && rd_covered((int)(p - row), y, ax, ay, bx, by, tt)) v |= bits << (16 * h);
        }
        if (v) atomicOr(words + w, v);                               // one atomic per word, as the rectangles
    }
}

// ---------------------------------------------------------------------------------------------- rectangles
// One workgroup per rectangle; a lane takes one 32-bit word of a row (two pixels) and issues one atomic for it.
__global__ void __launch_bounds__(RD_THREADS) rd_rects_kernel(const int32_t *__restrict__ rects, const double *__restrict__ anchors,
                                                              int64_t n_anchor, unsigned *__restrict__ words, int n_cam, int H, int W) {
    const int32_t *q = rects + (int64_t)blockIdx.x * 8;
    int64_t x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3];
    const int c = q[4], mode = q[5], a = q[6], bit = q[7];
    if (c < 0 || c >= n_cam || bit < 0 || bit > 15) return;
    if (a >= 0) {
        int ox, oy;
        if (!rd_anchor(anchors, n_anchor, a, ox, oy)) return;
        x0 += ox; x1 += ox; y0 += oy; y1 += oy;
    }
    if (x0 >= x1 || y0 >= y1) return;
    const int cx0 = (int)max(x0, (int64_t)0), cy0 = (int)max(y0, (int64_t)0);
    const int cx1 = (int)min(x1, (int64_t)W), cy1 = (int)min(y1, (int64_t)H);
    if (cx0 >= cx1 || cy0 >= cy1) return;
    const unsigned bits = 1u << bit;
    const int64_t plane = (int64_t)c * H * W;
    const int wpr = (cx1 - cx0) / 2 + 2;                              // words a row can touch
    const int64_t items = (int64_t)(cy1 - cy0) * wpr;
    for (int64_t it = threadIdx.x; it < items; it += RD_THREADS) {
        const int y = cy0 + (int)(it / wpr), k = (int)(it % wpr);
        const int64_t p0 = plane + (int64_t)y * W + cx0, p1 = plane + (int64_t)y * W + cx1;       // pixels [p0, p1)
        const int64_t w = (p0 >> 1) + k;
        if (w > ((p1 - 1) >> 1)) continue;
        const bool edge_row = (y == y0 || y == y1 - 1);
        unsigned v = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t p = 2 * w + h;
            if (p < p0 || p >= p1) continue;
            const int64_t x = cx0 + (p - p0);
            if (mode == 0 || edge_row || x == x0 || x == x1 - 1) v |= bits << (16 * h);
        }
        if (v) atomicOr(words + w, v);
    }
}

// ---------------------------------------------------------------------------------------------- text
// is pixel (px, py), relative to the run's cell origin (left, top), part of a glyph?
__device__ __forceinline__ bool rd_glyph_pixel(const uint8_t *__restrict__ text, const uint8_t *__restrict__ font, int start, int len,
                                               int s, int px, int py) {
    if (px < 0 || py < 0 || py >= 8 * s || px >= 6 * s * len) return false;
    const int i = px / (6 * s), col = (px - i * 6 * s) / s, row = py / s;
    int ch = text[start + i];
    if (ch < 32 || ch > 126) ch = '?';
    return (font[(ch - 32) * 8 + row] >> (5 - col)) & 1;
}

__global__ void __launch_bounds__(RD_THREADS) rd_text_kernel(const int32_t *__restrict__ runs, const uint8_t *__restrict__ text,
                                                             int64_t n_text, const uint8_t *__restrict__ font,
                                                             const double *__restrict__ anchors, int64_t n_anchor,
                                                             unsigned *__restrict__ words, int n_cam, int H, int W) {
    const int32_t *q = runs + (int64_t)blockIdx.x * 9;
    int64_t x = q[0], y = q[1];
    const int c = q[2], a = q[3], s = q[4], dil = q[5], bit = q[6], start = q[7], len = q[8];
    if (c < 0 || c >= n_cam || bit < 0 || bit > 15 || s < 1 || s > 64 || dil < 0 || dil > 1 || len <= 0 || start < 0 ||
        (int64_t)start + len > n_text)
        return;
    if (a >= 0) {
        int ox, oy;
        if (!rd_anchor(anchors, n_anchor, a, ox, oy)) return;
        x += ox; y += oy;
    }
    const int64_t left = x, top = y - 8 * s;                          // the run's cells: [left, left + 6 s len) x [top, y)
    const int64_t X0 = max(left - dil, (int64_t)0), X1 = min(left + (int64_t)6 * s * len + dil, (int64_t)W);
    const int64_t Y0 = max(top - dil, (int64_t)0), Y1 = min(y + dil, (int64_t)H);
    if (X0 >= X1 || Y0 >= Y1) return;
    const int wd = (int)(X1 - X0);
    const int64_t items = (Y1 - Y0) * wd;
    const unsigned bits = 1u << bit;
    const int64_t plane = (int64_t)c * H * W;
    for (int64_t it = threadIdx.x; it < items; it += RD_THREADS) {
        const int64_t py = Y0 + it / wd, px = X0 + it % wd;
        const int gx = (int)(px - left), gy = (int)(py - top);
        bool on = false;
        for (int v = -dil; v <= dil; ++v)
            for (int u = -dil; u <= dil; ++u) on = on || rd_glyph_pixel(text, font, start, len, s, gx + u, gy + v);
        if (on) rd_or_pixel(words, plane + py * W + px, bits);
    }
}

// ---------------------------------------------------------------------------------------------- compose
struct rd_norm {
    float mean[3], std[3];
};

// one channel of one pixel: include/retinanet_mi355x.h, rn_render_compose.  One fp32 rounding per line.
__device__ __forceinline__ unsigned rd_channel(float x, float mean, float std, unsigned m, int ch, bool dim) {
    float t = x * std;
    t = t + mean;
    t = t * 255.0f;
    t = t + 0.5f;
    t = floorf(t);
    t = fminf(fmaxf(t, 0.0f), 255.0f);
    float v = t / 255.0f;
    if (m) {
        if (m & RN_RENDER_PRIOR) v = ch == 2 ? 0.0f : 255.0f;
        if (m & RN_RENDER_CROP_EDGE) v = 255.0f;
        if (m & RN_RENDER_TRACK) v = ch == 0 ? 0.0f : (ch == 1 ? 200.0f : 25.0f);
        if (m & RN_RENDER_DET) v = ch == 0 ? 255.0f : 0.0f;
    }
    if (dim && !(m & RN_RENDER_IN_CROP)) v = 0.3f * v;
    if (m & (RN_RENDER_LABEL | RN_RENDER_LABEL_TEXT)) {
        const bool txt = m & RN_RENDER_LABEL_TEXT;
        const float a = txt ? 0.0f : v;
        const float b = txt ? 0.0f : ((m & RN_RENDER_LABEL) ? 1.0f : v);
        const float a7 = 0.7f * a;
        const float b3 = 0.3f * b;
        v = a7 + b3;
    }
    if (m & RN_RENDER_BANNER_EDGE) v = 1.0f;
    if (m & RN_RENDER_BANNER_TEXT) v = 0.0f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = v * 255.0f;
    v = v + 0.5f;
    return (unsigned)v;
}

// A lane takes four consecutive pixels of one row of one tile: 16-byte loads from the three planes and 8 bytes of mask when the
// row's addresses allow it (always when W is a multiple of 4), single loads otherwise and for the row's tail; twelve bytes out,
// as three dwords when aligned.  Tiles past n_cam are written as zeros.
__global__ void __launch_bounds__(RD_THREADS) rd_compose_kernel(const float *__restrict__ frames, rd_norm nm,
                                                                const uint16_t *__restrict__ mask, int dim, uint8_t *__restrict__ out,
                                                                int n_cam, int H, int W, int C, int64_t groups, int gpr) {
    const int64_t g = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (g >= groups) return;
    const int64_t row = g / gpr;                                      // tile * H + y
    const int x0 = (int)(g % gpr) * 4;
    const int tile = (int)(row / H), y = (int)(row % H);
    const int n = min(4, W - x0);
    const int64_t o = ((((int64_t)(tile / C) * H + y) * C + (tile % C)) * W + x0) * 3;             // byte offset in the canvas
    unsigned px[4][3];
    if (tile >= n_cam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j][0] = px[j][1] = px[j][2] = 0;
    } else {
        const int64_t hw = (int64_t)H * W;
        const float *f = frames + (int64_t)tile * 3 * hw + (int64_t)y * W + x0;
        const uint16_t *mp = mask + (int64_t)tile * hw + (int64_t)y * W + x0;
        float v[3][4];
        unsigned m[4];
        const bool full = n == 4;
        if (full && (((uintptr_t)f | (uintptr_t)(f + hw) | (uintptr_t)(f + 2 * hw)) & 15) == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float4 t = *reinterpret_cast<const float4 *>(f + ch * hw);
                v[ch][0] = t.x; v[ch][1] = t.y; v[ch][2] = t.z; v[ch][3] = t.w;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[ch][j] = j < n ? f[ch * hw + j] : 0.0f;
        }
        if (full && ((uintptr_t)mp & 7) == 0) {
            const uint2 t = *reinterpret_cast<const uint2 *>(mp);
            m[0] = t.x & 0xFFFFu; m[1] = t.x >> 16; m[2] = t.y & 0xFFFFu; m[3] = t.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = j < n ? mp[j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[j][ch] = rd_channel(v[ch][j], nm.mean[ch], nm.std[ch], m[j], ch, dim != 0);
    }
    uint8_t *dst = out + o;
    if (n == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned *d = reinterpret_cast<unsigned *>(dst);
        d[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
        d[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
        d[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                dst[3 * j] = (uint8_t)px[j][0];
                dst[3 * j + 1] = (uint8_t)px[j][1];
                dst[3 * j + 2] = (uint8_t)px[j][2];
            }
    }
}

// ---------------------------------------------------------------------------------------------- entry points
static bool rd_plane_ok(const void *mask, int n_cam, int H, int W) {
    return mask != nullptr && ((uintptr_t)mask & 3) == 0 && n_cam >= 1 && n_cam <= 65535 && H >= 1 && W >= 1 && H <= RN_RENDER_MAX_DIM &&
           W <= RN_RENDER_MAX_DIM;
}

extern "C" int rn_render_edges(const double *corners, const int32_t *cam, int64_t n, int thickness, int bit, uint16_t *mask,
                               int n_cam, int H, int W, void *stream) {
    if (n < 0 || n > (int64_t)(0x7FFFFFFF / 14) || thickness < 1 || thickness > 255 || bit < 0 || bit > 15 ||
        !rd_plane_ok(mask, n_cam, H, W))
        return RN_EINVAL;
    if (n > 0) {
        hipLaunchKernelGGL(rd_edges_kernel, dim3((unsigned)(n * 14)), dim3(RD_THREADS), 0, (hipStream_t)stream, corners, cam, thickness,
                           1u << bit, reinterpret_cast<unsigned *>(mask), n_cam, H, W);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_render_rects(const int32_t *rects, int64_t n, const double *anchors, int64_t n_anchor, uint16_t *mask, int n_cam,
                               int H, int W, void *stream) {
    if (n < 0 || n > 0x7FFFFFFF || n_anchor < 0 || n_anchor > 0x7FFFFFFF || (n_anchor > 0 && anchors == nullptr) ||
        !rd_plane_ok(mask, n_cam, H, W))
        return RN_EINVAL;
    if (n > 0) {
        hipLaunchKernelGGL(rd_rects_kernel, dim3((unsigned)n), dim3(RD_THREADS), 0, (hipStream_t)stream, rects, anchors, n_anchor,
                           reinterpret_cast<unsigned *>(mask), n_cam, H, W);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_render_text(const int32_t *runs, int64_t n, const uint8_t *text, int64_t n_text, const uint8_t *font,
                              const double *anchors, int64_t n_anchor, uint16_t *mask, int n_cam, int H, int W, void *stream) {
    if (n < 0 || n > 0x7FFFFFFF || n_text < 0 || n_text > 0x7FFFFFFF || n_anchor < 0 || n_anchor > 0x7FFFFFFF ||
        (n_anchor > 0 && anchors == nullptr) || (n > 0 && font == nullptr) || !rd_plane_ok(mask, n_cam, H, W))
        return RN_EINVAL;
    if (n > 0) {
        hipLaunchKernelGGL(rd_text_kernel, dim3((unsigned)n), dim3(RD_THREADS), 0, (hipStream_t)stream, runs, text, n_text, font, anchors,
                           n_anchor, reinterpret_cast<unsigned *>(mask), n_cam, H, W);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_render_compose(const float *frames, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                 const uint16_t *mask, int crops_present, uint8_t *out, int n_cam, int H, int W, int C,
                                 void *stream) {
    if (!rd_plane_ok(mask, n_cam, H, W) || C < 1 || C > n_cam || frames == nullptr || out == nullptr) return RN_EINVAL;
    const int R = (n_cam + C - 1) / C, gpr = (W + 3) / 4;
    const int64_t groups = (int64_t)R * C * H * gpr;
    if (groups > (int64_t)0x7FFFFFFF * RD_THREADS) return RN_EINVAL;
    rd_norm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    hipLaunchKernelGGL(rd_compose_kernel, dim3((unsigned)rn_blocks(groups, RD_THREADS)), dim3(RD_THREADS), 0, (hipStream_t)stream, frames,
                       nm, mask, crops_present, out, n_cam, H, W, C, groups, gpr);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
