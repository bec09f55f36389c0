"""CPU: the K-slice planner both weight-gradient launchers call (3d-playground_amd/csrc/conv_wgrad_plan.h) against recorded plans.  A
small host program with its own main (tests/wgrad_plan_check.cpp) is compiled around the header with g++ and prints the plan of every
case; what it prints must equal, exactly,
  * fp32 (tests/wgrad_cases.py): FP32_PLAN below -- per case (tile shape, tiles, K slices, pixels per slice, xcd_map, workgroups) at the
    native target of 2048 workgroups and at the split modes' 1536, as rn_conv_wgrad_plan reported them on the parent of the commit that
    introduced the header -- and the `expect` fields the cases carry;
  * bf16 (tests/wgrad_bf16_cases.py): PLAN and GROUP_PLAN, recorded on the same parent from wgrad_bf16_fill's arithmetic;
  * a few synthetic problems that reach the 2 GiB doubling loop and the refusal, recorded likewise.
The library's own rn_conv_wgrad_plan is held to the same fp32 record (host code: no GPU)."""
import os
import subprocess

import pytest

import wgrad_bf16_cases as bc
import wgrad_cases as wc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = (("native", 2048), ("split", 1536))

# name -> ((shape, tiles, splits, per_split, xcd_map, grid) native, the same in the split modes); recorded on the parent
FP32_PLAN = {
    "xcd-512-512-3x3-60x60": ((2, 144, 16, 704, 1, 2304), (2, 144, 16, 704, 1, 2304)),
    "xcd-surplus-256-384-3x3-70x88": ((2, 54, 39, 640, 1, 2160), (2, 54, 31, 800, 1, 1728)),
    "four-batches-512-512-3x3-59x59": ((2, 144, 16, 896, 1, 2304), (2, 144, 16, 896, 1, 2304)),
    "relu-64-64-3x3": ((0, 3, 7, 480, 0, 21), (0, 3, 7, 480, 0, 21)),
    "relu-64-256-1x1": ((1, 1, 7, 480, 0, 7), (1, 1, 7, 480, 0, 7)),
    "relu-128-128-3x3": ((2, 9, 7, 480, 0, 63), (2, 9, 7, 480, 0, 63)),
    "cout-64": ((0, 3, 1, 448, 0, 3), (0, 3, 1, 448, 0, 3)),
    "cout-65": ((2, 5, 1, 448, 0, 5), (2, 5, 1, 448, 0, 5)),
    "kflat-64": ((1, 1, 1, 448, 0, 1), (1, 1, 1, 448, 0, 1)),
    "kflat-68": ((2, 1, 1, 448, 0, 1), (2, 1, 1, 448, 0, 1)),
    "cout-1": ((0, 3, 1, 448, 0, 3), (0, 3, 1, 448, 0, 3)),
    "cin-4": ((1, 1, 1, 448, 0, 1), (1, 1, 1, 448, 0, 1)),
    "pixels-1": ((2, 1, 1, 32, 0, 1), (2, 1, 1, 32, 0, 1)),
    "pixels-15": ((2, 1, 1, 32, 0, 1), (2, 1, 1, 32, 0, 1)),
    "pixels-16": ((2, 1, 1, 32, 0, 1), (2, 1, 1, 32, 0, 1)),
    "pixels-17": ((2, 1, 1, 32, 0, 1), (2, 1, 1, 32, 0, 1)),
    "pixels-512-one-slice": ((2, 1, 1, 512, 0, 1), (2, 1, 1, 512, 0, 1)),
    "pixels-513-two-slices": ((2, 1, 2, 288, 0, 2), (2, 1, 2, 288, 0, 2)),
    "pixels-288": ((2, 1, 1, 288, 0, 1), (2, 1, 1, 288, 0, 1)),
    "pixels-289": ((2, 1, 1, 320, 0, 1), (2, 1, 1, 320, 0, 1)),
    "image-1x1-under-3x3": ((2, 9, 1, 32, 0, 9), (2, 9, 1, 32, 0, 9)),
    "s2-3x3-17x21": ((2, 9, 1, 224, 0, 9), (2, 9, 1, 224, 0, 9)),
    "s2-3x3-18x20": ((2, 9, 1, 192, 0, 9), (2, 9, 1, 192, 0, 9)),
    "s2-1x1-17x15": ((2, 2, 1, 160, 0, 2), (2, 2, 1, 160, 0, 2)),
    "stem-7x7-s2-kw8": ((0, 1, 2, 448, 0, 2), (0, 1, 2, 448, 0, 2)),
    "ldy-108-128": ((2, 18, 1, 160, 0, 18), (2, 18, 1, 160, 0, 18)),
    "ldy-72-96": ((2, 18, 1, 320, 0, 18), (2, 18, 1, 320, 0, 18)),
    "onehot-128-128-3x3-s1": ((2, 9, 4, 512, 0, 36), (2, 9, 4, 512, 0, 36)),
    "onehot-64-64-3x3-s2": ((0, 3, 2, 288, 0, 6), (0, 3, 2, 288, 0, 6)),
    "onehot-xcd-512-512-3x3-60x60": ((2, 144, 16, 704, 1, 2304), (2, 144, 16, 704, 1, 2304)),
}
# planner input row -> recorded output: the 2 GiB loop doubles the slices (the bf16 rule decides its XCD order afterwards, the fp32 rule
# drops its flag), a single image of more than 2 GiB is refused, a grouped range in the XCD order is not padded again, RN_WGRAD_BF16_XCD=0
SYNTHETIC = [
    ((1 << 22, 4, 768, 32, 1 << 16, 2, 1 << 22, 1 << 20, 1, 1, 0), (10944, 384, 1, 1536)),
    ((1 << 22, 16, 2048, 32, 1 << 16, 4, 1 << 22, 1 << 20, 0, 1, 0), (4096, 1024, 0, 16384)),
    ((4096, 1, 768, 32, 64, 2, 4096, (1 << 31) + 64, 1, 1, 0), None),
    ((4096, 1, 2048, 32, 64, 4, 4096, (1 << 31) + 64, 0, 1, 0), None),
    ((1 << 20, 4, 768, 32, 64, 2, 64, 1 << 24, 1, 1, 1), (5472, 192, 1, 768)),
    ((1 << 20, 32, 2048, 32, 64, 4, 64, 1 << 24, 0, 1, 0), (4096, 256, 0, 8192)),
    ((17672, 36, 768, 32, 512, 2, 8836, 2262016, 1, 0, 0), (832, 22, 0, 792)),
]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "3d-playground_amd", "csrc"),
                           os.path.join(REPO, "tests", "wgrad_plan_check.cpp"), "-o", exe])

    def run(rows):
        text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(rows), r.stdout
        return [None if ln == "refused" else tuple(int(v) for v in ln.split()) for ln in lines]
    return run


def fp32_tiles(c, shape):
    """Tile shape -> tiles, as wgrad_launch counts them (one batch entry)."""
    bm, bn = ((64, 256), (256, 64), (128, 128))[shape]
    return ((c.cout + bm - 1) // bm) * ((wc.kflat(c) + bn - 1) // bn)


def fp32_row(c, tiles, target):
    ho, wo = wc.out_hw(c)
    return (wc.pixels(c), tiles, target, 32, c.ldy, 4, ho * wo, c.H * c.W * c.cin * 4, 0, 1, 0)


def test_fp32_cases_match_the_record(planner):
    cases = wc.DENSE + wc.ONEHOT
    assert {c.name for c in cases} == set(FP32_PLAN)
    for k, (mode, target) in enumerate(TARGETS):
        got = planner([fp32_row(c, FP32_PLAN[c.name][k][1], target) for c in cases])
        for c, g in zip(cases, got):
            shape, tiles, splits, per_split, xcd_map, grid = FP32_PLAN[c.name][k]
            assert tiles == fp32_tiles(c, shape) and shape == c.expect["shape"], c.name
            assert g == (per_split, splits, xcd_map, grid), (c.name, mode, g)
            plan = dict(shape=shape, tiles=tiles, splits=splits, per_split=per_split, xcd_map=xcd_map, grid=grid, kernel=int(c.expect.get("once", False) and k))
            assert not wc.check_plan(c, plan, bool(k)), (c.name, mode, wc.check_plan(c, plan, bool(k)))


def test_bf16_cases_match_the_record(planner):
    assert set(bc.PLAN) == set(bc.BY_NAME)
    got = planner([bc.planner_row(c) for c in bc.CASES])
    for c, g in zip(bc.CASES, got):
        tiles, splits, per_split, xcd_map, blocks = bc.PLAN[c.name]
        assert tiles == bc.tiles(c) and g == (per_split, splits, xcd_map, blocks), (c.name, g)
        assert (splits - 1) * per_split < bc.pixels(c) <= splits * per_split and per_split % 32 == 0


def test_bf16_groups_match_the_record(planner):
    for name in bc.GROUPS:
        cs, shares = bc.group_cases(name)
        got = planner([bc.planner_row(c, s, pad8=True) for c, s in zip(cs, shares)])
        for c, s, g, rec in zip(cs, shares, got, bc.GROUP_PLAN[name]):
            assert rec[:2] == (s, bc.tiles(c)) and g == (rec[3], rec[2], rec[4], rec[5]), (c.name, g, rec)
            assert rec[5] % 8 == 0                                                     # every range starts at a multiple of 8


def test_bf16_cases_reach_what_they_are_named_for():
    """The properties the GPU cases exist for, read off the record."""
    tiles, splits, per_split, xcd_map, blocks = bc.PLAN["xcd-surplus-256-256-1x1-48x48"]
    assert xcd_map == 1 and splits % 8 != 0 and blocks == tiles * 16 > tiles * splits       # a padding group that returns early
    tiles, splits, per_split, xcd_map, blocks = bc.PLAN["plain-128-128-1x1-40x40"]
    assert tiles == 1 and splits > 1 and xcd_map == 0
    tiles, splits, per_split, xcd_map, blocks = bc.PLAN["table-reuse-128-512-3x3-94x94"]
    assert per_split > 768 and (per_split // 32 + 7) // 8 >= 4 and xcd_map == 1              # four table batches: both slots refilled
    assert [bc.pixels(bc.BY_NAME["pixels-%d" % n]) for n in (1, 31, 32, 33, 511, 512, 513)] == [1, 31, 32, 33, 511, 512, 513]
    assert bc.PLAN["pixels-512"][1:3] == (1, 512) and bc.PLAN["pixels-513"][1] == 2
    assert bc.kflat(bc.BY_NAME["cin-40-3x3"]) == 360 and bc.tiles(bc.BY_NAME["cout-130"]) == 2 * bc.tiles(bc.BY_NAME["cout-72-ldy-96"])
    zero = bc.GROUP_PLAN["share-zero"]
    assert zero[-1][0] == 0 and zero[-1][2] == 1 and zero[-1][5] > zero[-1][1] * zero[-1][2]   # share 0 -> one slice, range padded
    for name in bc.GROUPS:
        rec = bc.GROUP_PLAN[name]
        assert any(r[4] == 1 for r in rec) and any(r[4] == 0 and r[5] > r[1] * r[2] for r in rec)
    for c in bc.CASES:
        assert 4 * bc.pixels(c) < 2 ** 24 and c.ldy % 8 == 0 and c.cin % 8 == 0 and c.ldy >= c.cout


def test_synthetic_rows(planner):
    assert planner([row for row, _ in SYNTHETIC]) == [want for _, want in SYNTHETIC]


def test_library_plan_matches_the_record():
    """rn_conv_wgrad_plan (the launcher's own numbers, host code) reports the recorded plan for every fp32 case in every product mode."""
    from retinanet_mi355x import _hip, conv
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    before = conv.get_fp32_mfma()
    try:
        for c in wc.DENSE + wc.ONEHOT:
            for mode, k in (("native", 0), ("split", 1), ("split3", 1)):
                conv.set_fp32_mfma(mode)
                p = conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, wc.geom(c), have_amax=mode == "split3")
                assert (p["shape"], p["tiles"], p["splits"], p["per_split"], p["xcd_map"], p["grid"]) == FP32_PLAN[c.name][k], (c.name, mode, p)
    finally:
        conv.set_fp32_mfma(before)
