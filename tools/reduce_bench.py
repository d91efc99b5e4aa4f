"""Where the time of the step's final-reduction launch goes (gcl_reduce_jobs, csrc/linear.hip).

    python tools/reduce_bench.py [--iters 40] [--ring 4] [--out profiles/reduce_tail_kbench.txt]

The flagship step (baseline config, B = 64) queues 14 fused dense backwards, each with 512 partial records of
64 x 64 + 64 + 64 = 4224 floats and 512 slope partials: 121 MB to read in one launch.  This tool builds those 14 job
descriptions over synthetic partials and times the launch with HIP events, once as it is and once with every slope
partial pointer null (no scalar block at all).  The difference is what the scalar block costs ON TOP of the body blocks:
it is the last block dispatched, so whatever it takes beyond the body's tail is the launch's critical path.
Every launch reads another workspace of a ring (default 4 x 121 MB, past the 256 MB Infinity Cache), so nothing is
re-read from a cache.  Prints the medians and writes them to --out.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS, NPARTS, F = 14, 512, 64
REC = F * F + F + F


def main():
    import torch

    from graphcast_lite_amd import hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lib = hip.lib()
    dW = [torch.zeros(F, F, device=dev) for _ in range(JOBS)]
    db = [torch.zeros(F, device=dev) for _ in range(JOBS)]
    cs = [torch.zeros(F, device=dev) for _ in range(JOBS)]
    dslope = torch.zeros(1, device=dev)  # one shared PReLU slope, as in the model's conv stacks
    ring = []
    for r in range(a.ring):
        part = torch.randn(JOBS, NPARTS, REC, device=dev)
        spart = torch.randn(JOBS, NPARTS, device=dev, dtype=torch.float64)
        ring.append((part, spart))

    def jobs_of(part, spart, with_slope):
        arr = (hip.ReduceJob * JOBS)()
        for q in range(JOBS):
            j = arr[q]
            j.part, j.pstride, j.nparts = part[q].data_ptr(), REC, NPARTS
            for t, (out, poff, count, pld, cols, ldo) in enumerate(((dW[q], 0, F * F, F, F, F), (db[q], F * F, F, F, F, 0),
                                                                    (cs[q], F * F + F, F, F, F, 0))):
                s = j.seg[t]
                s.out, s.poff, s.count, s.pld, s.cols, s.ldo, s.acc = out.data_ptr(), poff, count, pld, cols, ldo, 0
            if with_slope:
                j.spart, j.sout, j.ns = spart[q].data_ptr(), dslope.data_ptr(), NPARTS
        return arr

    def measure(with_slope):
        arrs = [jobs_of(p, s, with_slope) for p, s in ring]
        ts = []
        for it in range(a.iters + 3):
            arr = arrs[it % a.ring]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip._check(lib.gcl_reduce_jobs(C.cast(arr, C.c_void_p), JOBS, hip._stream()))
            e1.record()
            e1.synchronize()
            if it >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    mb = JOBS * NPARTS * REC * 4 / 1e6
    lines = [f"gcl_reduce_jobs: {JOBS} jobs x {NPARTS} records x {REC} floats = {mb:.1f} MB per launch, ring of {a.ring}, "
             f"{a.iters} launches each (HIP events, one launch between two events; median / min in us)"]
    for name, ws in (("as queued by the step (slope partials of every job)", True), ("every spart null (no scalar block)", False)):
        med, lo = measure(ws)
        lines.append(f"{name:55s} {med:8.1f} {lo:8.1f}   {mb / med:6.2f} TB/s at the median")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
