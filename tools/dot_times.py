#!/usr/bin/env python3
"""y = A x with w . y and y . y from the same pass, against what a caller does
without it: the execute, then torch.dot(w, y) and torch.dot(y, y).

For each (matrix, format) one plan is built; in ONE process, on that plan,
everything device-resident and on one side stream, these are timed:

  execute     spmv_time                       (the plain product, for reference
                                               and for parent / new comparisons)
  yardstick   plan.execute(async) ; torch.dot(w, y) ; torch.dot(y, y), `iters`
              times between two events on the plan's stream -- what a Krylov
              loop runs today.  THE yardstick: the new code is never its own.
  dot_calls   plan.execute_dot(async, device dots), `iters` times between the
              same kind of events -- the same host-side call overhead as the
              yardstick's execute
  dot         spmv_time_dot                   (the launches alone, as spmv_time)

Rounds are interleaved (every variant once per round, so drift and neighbours
hit all of them alike) and the minimum per variant is kept; the spread
(max / min over the rounds) is recorded per variant.  Compare only within one
process and one plan, never across runs (placements move a kernel by up to
~10 %).  A package without execute_dot (the parent commit's,
through SPMV_PACKAGE_ROOT) gives the execute and yardstick columns only.

One JSON line per (matrix, format): path (spmv_dot_path), ms_* (min per
call), spread_*, dot_vs_yardstick = ms_dot_calls / ms_yardstick, and
saved_bytes = 16 m (y read twice, w once, less the w[r] the epilogue reads:
24 m - 8 m), the traffic a fused path no longer moves.

Matrices:
  banded64   64 diagonals, 2 M rows: dia, ell, csr (csr_slabx, 16 lanes)
  uniform16  16 per row, 10 M x 10 M (config 2): csr (csr_slab2, 4 lanes), ell,
             bin (generic path)
  powerlaw   1 M power-law rows: csr (csr_adaptive)
  small      16 per row, 10 K rows: csr (launch-bound)

  python tools/dot_times.py [--out FILE] [--scale 1.0] [--rounds 7] [--iters 5] [--only NAMES]
"""
import argparse
import json
import os
import sys

import torch

# SPMV_PACKAGE_ROOT: the directory that holds another build of the package (the
# parent commit's singlespmv_amd/ with its library), for parent / new comparisons
sys.path.insert(0, os.environ.get("SPMV_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import singlespmv_amd as sp  # noqa: E402


def matrices(scale):
    m = int(2_000_000 * scale)
    yield "banded64", m, lambda: sp.generate_csr(sp.gen_spec("banded", m, band_lo=-32, band_hi=31, seed=4)), \
        ("dia", "ell", "csr")
    m2 = int(10_000_000 * scale)
    yield "uniform16", m2, lambda: sp.generate_csr(sp.gen_spec("uniform", m2, per_row=16, seed=2)), ("csr", "ell", "bin")
    m3 = int(1_000_000 * scale)
    yield "powerlaw", m3, lambda: sp.generate_csr(sp.gen_spec("powerlaw", m3, max_len=10000, alpha=2.0, seed=3)), \
        ("csr",)
    m4 = 10_000
    yield "small", m4, lambda: sp.generate_csr(sp.gen_spec("uniform", m4, per_row=16, seed=5)), ("csr",)


def time_plan(plan, m, rounds, iters, have_dot):
    """{variant: [ms per call, one per round]} on a side stream."""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    w = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    dots = torch.zeros(2, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.set_stream(side)

    def between_events(body, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record(side)
            for _ in range(n):
                body()
            b.record(side)
        b.synchronize()
        return a.elapsed_time(b) / n

    def yardstick():
        plan.execute(x, y, async_=True)
        torch.dot(w, y)
        torch.dot(y, y)

    variants = {"execute": lambda n: plan.time(x, y, n) / n, "yardstick": lambda n: between_events(yardstick, n)}
    if have_dot:
        variants["dot_calls"] = lambda n: between_events(lambda: plan.execute_dot(x, y, w, dots=dots, async_=True), n)
        variants["dot"] = lambda n: plan.time_dot(x, y, w, dots, n) / n
    seen = {v: [] for v in variants}
    try:
        for r in range(rounds + 1):  # round 0: warm-up (code objects loaded, partials allocated)
            for v, run in variants.items():
                ms = run(iters if r else 1)
                if r:
                    seen[v].append(ms)
    finally:
        side.synchronize()
        plan.set_stream(None)
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = the sizes above)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    a = ap.parse_args()
    have_dot = hasattr(sp.Plan, "execute_dot")  # the parent's package has none
    out = open(a.out, "a") if a.out else sys.stdout
    for name, m, gen, fmts in matrices(a.scale):
        if a.only and name not in a.only.split(","):
            continue
        rp, col, val = gen()
        for fmt in fmts:
            plan = sp.Plan.from_csr(m, m, rp, col, val, fmt)
            info = plan.info()
            seen = time_plan(plan, m, a.rounds, a.iters, have_dot)
            rec = {"matrix": name, "m": m, "nnz": int(rp[-1]), "format": info["format"], "kernel": info["kernel"],
                   "path": plan.dot_path() if have_dot else None, "package": os.path.dirname(os.path.abspath(sp.__file__)),
                   "bytes_execute": info["algo_bytes"], "saved_bytes": 16 * m, "rounds": a.rounds, "iters": a.iters}
            for v, ms in seen.items():
                rec[f"ms_{v}"] = round(min(ms), 5)
                rec[f"spread_{v}"] = round(max(ms) / min(ms), 3)
            if have_dot:
                rec["dot_vs_yardstick"] = round(min(seen["dot_calls"]) / min(seen["yardstick"]), 4)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            plan.destroy()
            torch.cuda.empty_cache()
        del rp, col, val
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
