#!/usr/bin/env python3
"""4K frame intake at the loader's size: 18 cameras x 2160x3840 uint8.

  frame_ingest_half   time per call and TB/s of algorithmic bytes (per OUTPUT pixel 12 B read + 16 B NHWC4 / 12 B NCHW written,
                      + 3 B with the reduced uint8 frame kept), beside ops.frame_ingest on 18 x 1080p measured in the same
                      run (3 B read + 16 / 12 B written per pixel) -- that op is the yardstick
  time stamps         stream time by HIP events around ops.parse_frame_timestamps (one launch, tables on the device, no copy),
                      and the numpy restatement of the reference's loop (tests/frames4k_cases.py) on this machine's CPU
Medians of CALLS calls after WARMUP; the times include the output allocation.
    python tools/bench_frames4k.py [--out profiles/frames4k_bench.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)
import frames4k_cases as fc                       # noqa: E402
import timestamp_utilities as tsu                 # noqa: E402
from retinanet_mi355x import ops                  # noqa: E402

CALLS, WARMUP, B, H2, W2 = 30, 5, 18, 2160, 3840


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us), min(us)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "frames4k_bench.txt")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    say("4K frame intake on %s (%s, %d CUs): %d frames of %dx%d, medians (minima) of %d calls"
        % (prop.name, prop.gcnArchName, prop.multi_processor_count, B, H2, W2, CALLS))
    f4k = torch.randint(0, 256, (B, H2, W2, 3), dtype=torch.uint8, device=dev)
    H, W = H2 // 2, W2 // 2
    f1080 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    px = B * H * W
    say("%-44s %10s %10s %8s %10s" % ("op", "us", "(min us)", "MB", "TB/s"))
    for nhwc4 in (True, False):
        lay, wr = ("NHWC4", 16) if nhwc4 else ("NCHW", 12)
        for name, fn, nbytes in (
                ("frame_ingest       18 x 1080p  " + lay, lambda: ops.frame_ingest(f1080, nhwc4=nhwc4), px * (3 + wr)),
                ("frame_ingest_half  18 x 4K     " + lay, lambda: ops.frame_ingest_half(f4k, nhwc4=nhwc4), px * (12 + wr)),
                ("frame_ingest_half  18 x 4K +u8 " + lay, lambda: ops.frame_ingest_half(f4k, nhwc4=nhwc4, keep_u8=True), px * (12 + wr + 3))):
            med, low = timed(fn)
            say("%-44s %10.1f %10.1f %8.1f %10.2f" % (name, med, low, nbytes / 1e6, nbytes / med / 1e6))
    # time stamps: a strip of 30 x 247 pixels (13 cells of 19 x 30) at the loader's place in a 4K frame
    geom = fc.geometry(19, 30, 13, x0=25, y0=20)
    tab = fc.table(geom)
    strips = np.stack([fc.render(fc.stamp_text(d, 13), geom, 64, 320) for d in fc.random_digits(B, 12, seed=7)])
    f4k[:, :64, :320] = torch.from_numpy(strips).to(dev)
    reader = tsu.TimestampReader([(geom, tab)], B, device=dev)
    want = fc.parse_frames(list(strips), [(geom, tab)])
    times, status = reader(f4k)
    assert np.array_equal(times.cpu().numpy(), want["times"]) and (status.cpu().numpy() == fc.READ).all()
    med, low = timed(lambda: ops.parse_frame_timestamps(f4k, (reader.geometry, reader.table), prev=reader.prev))
    say("%-44s %10.1f %10.1f   stream time by HIP events, one launch" % ("parse_frame_timestamps 18 x 4K, 13 x (19x30)", med, low))
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        fc.parse_frames(list(strips), [(geom, tab)])
        host.append((time.perf_counter() - t0) * 1e6)
    say("%-44s %10.1f              the numpy restatement on the host, 18 strips" % ("", statistics.median(host)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
