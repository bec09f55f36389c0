#!/usr/bin/env python3
"""Generate tests/golden/track_stitch.npz from the reference's shipped tracking output -- build container only.

``3D_tracking_results.csv`` of the reference checkout is data its tracker wrote.  The shipped file predates the last column of
the results template (the per-camera time-stamp bias, which the parser indexes), so a temporary copy gets that column -- the
header cell naming the one camera the file holds and a bias of 0.0 per row -- and is parsed with this repository's
``Data_Reader`` (its own parser; the constructor is host code and needs no device).  The data is packed by tracklet
(``track_stitch.pack_tracklets``) and run through the plain restatement of tests/stitch_cases.py with the default parameters.
The file holds the packed rows (ids, offsets, cols, direction) and the restatement's end points, candidate lists, compressed
matrices, links, chains and fill rows.  Nothing of the reference is imported or executed.  This script refuses to run without
the reference and is never executed on the GPU box.

    python tools/make_golden_track_stitch.py [--out DIR]
"""
import csv
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "3d-playground_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

REF = "/root/reference"
SOURCE = "3D_tracking_results.csv"


def main():
    out = os.path.join(REPO, "tests", "golden")
    argv = sys.argv[1:]
    if "--out" in argv:
        out = os.path.abspath(argv[argv.index("--out") + 1])
    path = os.path.join(REF, SOURCE)
    if not os.path.isfile(path):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % REF)
    import datareader
    import stitch_cases as sc
    import track_stitch
    with tempfile.TemporaryDirectory() as tmp:
        full = os.path.join(tmp, SOURCE)
        with open(path, "r", newline="") as src, open(full, "w", newline="") as dst:
            writer = csv.writer(dst)
            for row in csv.reader(src):
                if len(row) == 45:
                    row = row + (["ts_bias for cameras ['p1c1']"] if row[0] == "Frame #" else ["[0.0]"])
                writer.writerow(row)
        reader = datareader.Data_Reader(full, None)
    pk = track_stitch.pack_tracklets(reader.data)
    got = sc.run_all(pk["ids"], pk["offsets"], pk["cols"], pk["direction"])
    os.makedirs(out, exist_ok=True)
    keep = ("ep", "cand", "ncand", "Wc", "next", "prev", "link_cost", "root", "rank", "new_id", "count", "prefix", "fields", "time",
            "link", "side")
    np.savez_compressed(os.path.join(out, "track_stitch.npz"), ids=pk["ids"], offsets=pk["offsets"], cols=pk["cols"],
                        direction=pk["direction"], frame=pk["frame"], **{k: got[k] for k in keep})
    links = int((got["next"] >= 0).sum())
    print("%d tracklets, %d rows, %d links, %d chains of more than one, %d new rows" %
          (len(pk["ids"]), len(pk["cols"]), links, len(set(got["root"][got["next"] >= 0].tolist())), len(got["time"])))


if __name__ == "__main__":
    main()
