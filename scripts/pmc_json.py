"""Turn two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over bench.py into the per-launch HBM
traffic summary bench.py --full reads back into its roofline (profiles/*_pmc.json).

usage: pmc_json.py FETCH_DIR WRITE_DIR CONFIG BLOCK_SIZE X_STORAGE ALG_BYTES OUT

gfx950 correction (MI355X_MICROARCH.md, HBM / rocprofv3): FETCH_SIZE counts half the bytes the
TCC actually fetched, so HBM read bytes = 2 x FETCH_SIZE (kB) x 1024; WRITE_SIZE is taken as is.
Steady state = the mean of the last two dispatches (the timed sweeps; the earlier ones are the
burn-in of a fresh chain, whose change lists are larger).
"""
import csv
import glob
import json
import os
import sys


def per_dispatch(d, counter):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                kn = r.get("Kernel_Name", "")
                if r.get("Counter_Name") == counter and ("k_sweep<" in kn or "k_sweep_solve<" in kn or "k_sweep_stream<" in kn):
                    rows.append((int(r.get("Dispatch_Id", 0) or 0), float(r["Counter_Value"]), kn))
    rows.sort()
    if any("k_sweep_stream<" in k for _, _, k in rows) and not any("k_sweep_solve<" in k for _, _, k in rows):
        # the two-kernel sweep with only the streaming kernel profiled (--kernel-include-regex
        # k_sweep_stream): the counters are the device's TCC totals over its dispatch, which the solver
        # kernel's run lies within (launched first, finished before the streamers' end)
        return [v for _, v, k in rows], "k_sweep_stream (counters over the two-kernel sweep)"
    if any("k_sweep_stream<" in k for _, _, k in rows):
        # the two-kernel sweep: k_sweep_solve and k_sweep_stream of one sweep are launched back to
        # back (consecutive dispatch ids); a sweep's traffic is the sum of the pair
        sv = [v for _, v, k in rows if "k_sweep_solve" in k]
        tv = [v for _, v, k in rows if "k_sweep_stream" in k]
        return [a + b for a, b in zip(sv, tv)], "k_sweep_solve + k_sweep_stream"
    return [v for _, v, _ in rows], (rows[0][2] if rows else "?")


def main():
    fdir, wdir, cfg, B, xs, alg, out = sys.argv[1:8]
    fk, kname = per_dispatch(fdir, "FETCH_SIZE")
    wk, _ = per_dispatch(wdir, "WRITE_SIZE")
    if not fk or not wk:
        sys.exit("no k_sweep dispatches in the PMC output")
    # PMC_GROUP = launches per sweep (column-shard exchange segments: E launches of the marker loop per
    # sweep); the steady state is then the mean of the last two sweeps' sums
    grp = int(os.environ.get("PMC_GROUP", "1"))
    if grp > 1:
        fk = [sum(fk[i:i + grp]) for i in range(len(fk) % grp, len(fk), grp)]
        wk = [sum(wk[i:i + grp]) for i in range(len(wk) % grp, len(wk), grp)]
    ss_f = sum(fk[-2:]) / len(fk[-2:])
    ss_w = sum(wk[-2:]) / len(wk[-2:])
    d = {
        "config": cfg, "block_size": int(B), "x_storage": xs, "kernel": kname[:60],
        "dispatches": len(fk),
        "fetch_size_kb_per_dispatch": fk, "write_size_kb_per_dispatch": wk,
        "steady_state_fetch_kb": ss_f, "steady_state_write_kb": ss_w,
        "hbm_bytes_per_launch": (2.0 * ss_f + ss_w) * 1024.0,
        "algorithmic_bytes_per_launch": float(alg),
        "note": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes of bench.py --steps 2 --warmup 10; "
                "gfx950 correction FETCH_SIZE x2 (MI355X_MICROARCH.md HBM); steady state = mean of the last "
                "two (timed) dispatches",
    }
    with open(out, "w") as fh:
        json.dump(d, fh, indent=1)
    print(f"{out}: hbm {d['hbm_bytes_per_launch']:.4g} B/launch = "
          f"{d['hbm_bytes_per_launch'] / float(alg):.3f} x algorithmic")


if __name__ == "__main__":
    main()
