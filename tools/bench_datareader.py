#!/usr/bin/env python3
"""Time Data_Reader.reinterpolate + write_to_file on a generated 18-camera tracking file against the plain restatement
(tests/datareader_cases.py) in the same run, device time apart from host packing and CSV formatting.  Reported, not a gate.

    python tools/bench_datareader.py [--frames 400] [--objects 120] [--hz 30] [--out profiles/datareader_gpu.txt]
"""
import argparse
import csv
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)

import datareader_cases as dc                # noqa: E402
import datareader                            # noqa: E402
import homography                            # noqa: E402
import results_csv                           # noqa: E402


def clock(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--objects", type=int, default=120)
    ap.add_argument("--hz", type=float, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s)
        lines.append(s)
    names, P, _ = dc.cameras(18)
    hg = homography.Homography()
    hg.correspondence = {n: {"P": P[i]} for i, n in enumerate(names)}
    hg.default_correspondence = names[0]
    text = dc.tracking_csv(seed=21, n_frames=args.frames, n_objs=args.objects, n_cams=18)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.csv"), os.path.join(tmp, "out.csv")
        with open(src, "w", newline="") as f:
            f.write(text)
        t_load, dr = clock(lambda: datareader.Data_Reader(src, hg))
        rows_in = sum(len(f) for f in dr.data)
        say("Data_Reader on %s: %d rows in %d frames, 18 cameras, resampled to %g Hz" % (torch.cuda.get_device_name(0), rows_in,
                                                                                       len(dr.data), args.hz))
        say("load (host csv parser)                          : %9.1f ms" % (t_load * 1e3))
        start = [dict(f) for f in dr.data]
        # the pieces of reinterpolate
        t_walk, (inst_a, inst_time) = clock(lambda: (setattr(dr, "d_idx", 0), dr._walk(args.hz))[1])
        t_pack, pk = clock(lambda: datareader.pack_frames(dr.data))
        packed = (pk["offsets"], pk["ids"], pk["fields"], pk["frame_ts"], inst_a, inst_time)
        datareader.resample_packed(*packed, dev)                                               # warm-up: library load, allocator
        t_dev, got = clock(lambda: datareader.resample_packed(*packed, dev), args.reps)
        d_off, d_ids, d_fields, d_ts, d_a, d_time = datareader._upload(dev, [packed[0], packed[1], packed[2], packed[3],
                                                                             np.asarray(inst_a, np.int32), np.asarray(inst_time)])

        def launches():
            from retinanet_mi355x import ops
            mate, st = ops.reinterp_mate(d_off, d_ids)
            _, prefix, st = ops.reinterp_offsets(d_off, mate, d_a, status=st)
            return ops.reinterp_rows(d_off, d_ts, d_fields, mate, d_a, d_time, prefix, len(got[1]), status=st)
        t_kern, _ = clock(launches, args.reps)
        dr.d_idx = 0
        t_all, _ = clock(lambda: dr.reinterpolate(frequency=args.hz, save=None))
        rows_out = sum(len(f) for f in dr.data)
        say("reinterpolate -> %d instants, %d rows" % (len(dr.data), rows_out))
        say("  walk over instants (host, serial)             : %9.1f ms" % (t_walk * 1e3))
        say("  pack data into arrays (host)                  : %9.1f ms" % (t_pack * 1e3))
        say("  upload + 4 launches + copy back               : %9.3f ms   (the launches alone: %.3f ms)" % (t_dev * 1e3, t_kern * 1e3))
        say("  whole call, with the rebuild of the dicts     : %9.1f ms" % (t_all * 1e3))
        # the pieces of write_to_file
        items = [o for f in dr.data for o in f.values()]
        fields = [[o[k] for k in dc.FIELDS] for o in items]
        direction, cams = [o["direction"] for o in items], [o["camera"] for o in items]
        datareader.project_rows(hg, fields, direction, cams, dev)
        t_proj, _ = clock(lambda: datareader.project_rows(hg, fields, direction, cams, dev), args.reps)
        t_rows, rows = clock(dr.file_rows)

        def write(rows_):
            with open(out, "w") as f:
                csv.writer(f, delimiter=",").writerows([results_csv.RESULTS_HEADER] + rows_)
        t_csv, _ = clock(lambda: write(rows))
        t_write, _ = clock(lambda: dr.write_to_file(save_file=out))
        say("write_to_file -> %d rows" % len(rows))
        say("  upload + rn_track_rows + copy back            : %9.3f ms" % (t_proj * 1e3))
        say("  rows as Python cells (results_rows, with the above): %6.1f ms" % (t_rows * 1e3))
        say("  csv.writer over the cells                     : %9.1f ms" % (t_csv * 1e3))
        say("  whole call                                    : %9.1f ms" % (t_write * 1e3))
        with open(out, newline="") as f:
            written = f.read()
    t_ref_i, want = clock(lambda: dc.reinterpolate(start, args.hz))
    t_ref_w, want_text = clock(lambda: dc.file_text(want, dr.cameras, names, P))
    same = dc.dump(dr.data).tobytes() == dc.dump(want).tobytes()
    g, w = dc.parse(written), dc.parse(want_text)
    cols = list(dc.NUMERIC_COLS)
    dev_px = max((abs(float(a[c]) - float(b[c])) for a, b in zip(g[1:], w[1:]) for c in cols), default=0.0)
    strings = len(g) == len(w) and all(a[c] == b[c] for a, b in zip(g, w) for c in dc.STRING_COLS)
    say("restatement (plain Python / NumPy, CPU): reinterpolate %.1f ms, rows + text %.1f ms" % (t_ref_i * 1e3, t_ref_w * 1e3))
    say("same data bits: %s   same string cells: %s   largest image-cell deviation: %.3e px" % (same, strings, dev_px))
    host = t_all - t_dev + t_write - t_proj
    say("device share of reinterpolate + write_to_file: %.1f %%; the rest is Python: dict packing and rebuilding, cell formatting"
        % (100.0 * (t_dev + t_proj) / (t_all + t_write)) + (" -- formatting dominates" if host > t_dev + t_proj else ""))
    say("(the reference's write_to_file makes two single-box homography calls and five .item() reads per row; it is not run here)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
