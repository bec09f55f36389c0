// Host check of the fused 1x1 backward kernel's LDS index arithmetic (3d-playground_amd/csrc/conv_bwd_1x1_geom.h): every thread of
// every access is enumerated.  Stores must tile their plane images exactly once; every read must stay inside its image, find the
// element the MFMA operand layout wants, and be free of bank conflicts inside the lane groups the LDS serves together.
// Prints "ok <checks>" and exits 0, or the first violation and exits 1.  Built and run by tests/test_bwd_fused_index_ranges.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "conv_bwd_1x1_geom.h"

using G = Bwd1x1Geom;
static long checks = 0;
#define REQUIRE(c, ...)                       \
    do {                                      \
        ++checks;                             \
        if (!(c)) {                           \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                \
            std::exit(1);                     \
        }                                     \
    } while (0)

int main() {
    // ---- stores: where element (row, col) of a plane lives (byte address of its fp16), each byte written once
    std::vector<int> dy_at(G::DY_IMG / 2, -1), x_at(G::X_IMG / 2, -1);      // fp16 slot -> row * cols + col
    for (int tid = 0; tid < 256; ++tid) {
        for (int i = 0; i < 4; ++i) {
            const int a = G::dy_wr(tid, i), row = G::dy_pixel(tid, i);
            REQUIRE(a >= 0 && a + 8 <= G::DY_IMG && (a & 7) == 0 && row >= 0 && row < G::WK, "dy_wr tid %d i %d -> %d", tid, i, a);
            for (int j = 0; j < 4; ++j) {
                REQUIRE(dy_at[a / 2 + j] == -1, "dy plane byte %d written twice", a + 2 * j);
                dy_at[a / 2 + j] = row * G::CO + 4 * (tid & 63) + j;
            }
        }
        const int a = G::x_wr(tid), row = G::x_pixel(tid);
        REQUIRE(a >= 0 && a + 8 <= G::X_IMG && (a & 7) == 0 && row >= 0 && row < G::WK, "x_wr tid %d -> %d", tid, a);
        for (int j = 0; j < 4; ++j) {
            REQUIRE(x_at[a / 2 + j] == -1, "x plane byte %d written twice", a + 2 * j);
            x_at[a / 2 + j] = row * G::CI + 4 * (tid & 15) + j;
        }
    }
    for (int v : dy_at) REQUIRE(v >= 0, "a dy plane slot is never written");
    for (int v : x_at) REQUIRE(v >= 0, "an x plane slot is never written");
    // ds_write_b64 is served in four runs of 16 lanes over 32 banks of 4 bytes
    for (int w = 0; w < 4; ++w)
        for (int i = 0; i < 4; ++i)
            for (int run = 0; run < 4; ++run) {
                std::set<int> banks;
                for (int l = 16 * run; l < 16 * run + 16; ++l) {
                    const int a = G::dy_wr(64 * w + l, i);
                    banks.insert((a / 4) % 32);
                    banks.insert((a / 4 + 1) % 32);
                }
                REQUIRE(banks.size() == 32, "dy_wr bank conflict wave %d i %d run %d", w, i, run);
            }

    // ---- transposing reads (weight gradient): lane (g, q, pp) supplies 4 columns of one pixel; lane j of the 16-lane group then holds
    // column j of the group's 4 pixels x 16 columns.  Operand element [i = lane & 31][k = 8 (lane >> 5) + 4 rd + kk].
    for (int wave = 0; wave < 4; ++wave)
        for (int t = 0; t < 2; ++t)
            for (int rd = 0; rd < 2; ++rd) {
                for (int half = 0; half < 2; ++half) {              // served in two halves of 32 lanes, 64 banks
                    std::set<int> banks_dy, banks_x;
                    for (int lane = 32 * half; lane < 32 * half + 32; ++lane) {
                        const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
                        const int row = 8 * (g >> 1) + 4 * rd + q;                  // pixel k = 8 (lane >> 5) + 4 rd + q
                        const int a = G::dy_tr(wave, t, rd, lane);
                        REQUIRE(a >= 0 && a + 8 <= G::DY_IMG && (a & 7) == 0, "dy_tr range");
                        for (int j = 0; j < 4; ++j)
                            REQUIRE(dy_at[a / 2 + j] == row * G::CO + 64 * wave + 32 * t + 16 * (g & 1) + 4 * pp + j,
                                    "dy_tr wave %d t %d rd %d lane %d finds the wrong element", wave, t, rd, lane);
                        banks_dy.insert((a / 4) % 64);
                        banks_dy.insert((a / 4 + 1) % 64);
                        if (wave == 0) {
                            const int b = G::x_tr(t, rd, lane);
                            REQUIRE(b >= 0 && b + 8 <= G::X_IMG && (b & 7) == 0, "x_tr range");
                            for (int j = 0; j < 4; ++j)
                                REQUIRE(x_at[b / 2 + j] == row * G::CI + 32 * t + 16 * (g & 1) + 4 * pp + j,
                                        "x_tr t %d rd %d lane %d finds the wrong element", t, rd, lane);
                            banks_x.insert((b / 4) % 64);
                            banks_x.insert((b / 4 + 1) % 64);
                        }
                    }
                    REQUIRE(banks_dy.size() == 64, "dy_tr bank conflict wave %d t %d rd %d half %d", wave, t, rd, half);
                    if (wave == 0) REQUIRE(banks_x.size() == 64, "x_tr bank conflict t %d rd %d half %d", t, rd, half);
                }
            }

    // ---- data gradient: ds_read_b128 of row lane & 15, channels 32 kb + 8 (lane >> 4) .. + 7
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int kb = 0; kb < 8; ++kb) {
        for (int lane = 0; lane < 64; ++lane) {
            const int a = G::dy_a(lane, kb);
            REQUIRE(a >= 0 && a + 16 <= G::DY_IMG && (a & 15) == 0, "dy_a range");
            REQUIRE(a == (G::dy_a(lane, 0) ^ (kb << 6)), "dy_a(lane, kb) != dy_a(lane, 0) ^ (kb << 6)");
            for (int j = 0; j < 8; ++j)
                REQUIRE(dy_at[a / 2 + j] == (lane & 15) * G::CO + 32 * kb + 8 * (lane >> 4) + j, "dy_a lane %d kb %d finds the wrong element", lane, kb);
        }
        for (int gi = 0; gi < 4; ++gi) {
            std::set<int> slots;
            for (int i = 0; i < 16; ++i) slots.insert((G::dy_a(groups[gi][i], kb) / 16) % 16);
            REQUIRE(slots.size() == 16, "dy_a bank conflict kb %d group %d", kb, gi);
        }
    }

    // ---- dx stage: the four waves' results tile [16 pixels][64 channels] once; thread tid reads pixel tid >> 4, channels 4 (tid & 15) .. + 3
    std::vector<int> st_at(G::STAGE / 4, -1);
    for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int a = G::st_wr(wave, lane, r);
                REQUIRE(a >= 0 && a + 4 <= G::STAGE && (a & 3) == 0 && st_at[a / 4] == -1, "st_wr wave %d lane %d r %d -> %d", wave, lane, r, a);
                st_at[a / 4] = (4 * (lane >> 4) + r) * G::CI + 16 * wave + (lane & 15);
            }
    for (int tid = 0; tid < 256; ++tid) {
        const int a = G::st_rd(tid);
        REQUIRE(a >= 0 && a + 16 <= G::STAGE && (a & 15) == 0, "st_rd range");
        for (int j = 0; j < 4; ++j) REQUIRE(st_at[a / 4 + j] == (tid >> 4) * G::CI + 4 * (tid & 15) + j, "st_rd tid %d finds the wrong element", tid);
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
