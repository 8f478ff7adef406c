#!/usr/bin/env python3
"""y = alpha * A x + beta * y against the plain execute, on the same plans.

For each (matrix, format) one plan is built; in ONE process, on that plan,
everything device-resident, three calls are timed:

  execute   spmv_time                              (beta = 0, the yardstick)
  axpby     spmv_time_axpby at (alpha, beta) = (-2.5, 0.75), the plan's own path
  generic   the same call with the generic route forced (probe build only:
            SPMV_LAUNCH_AXPBY_GENERIC=1, read at every launch) -- the plan's
            kernels into the scratch vector, then one axpby pass

Rounds are interleaved (every variant once per round, so drift and neighbours
hit all of them alike) and the minimum per variant is kept.  Compare only
within one process and one plan, never across runs (placements move a kernel
by up to ~10 %).

One JSON line per (matrix, format):
  path                    spmv_axpby_path of the plan
  ms_execute, ms_axpby, ms_generic   min ms per call (ms_generic: null
                          without the probe build)
  bytes_execute           spmv_plan_info.algo_bytes
  bytes_fused / _generic  the byte model: + 8 m (y0 read in the epilogue) /
                          + 32 m (t written and read, y read and written)
  gbs_*                   model bytes / time

Matrices:
  banded64   64 diagonals, 2 M rows: dia, ell, csr (csr_slabx)
  uniform16  16 per row, 10 M x 10 M (config 2): csr (csr_slab2), ell, bin
  powerlaw   5 M power-law rows (config 3): csr (csr_adaptive), bin

  python tools/axpby_times.py [--out FILE] [--scale 1.0] [--rounds 7] [--iters 5] [--only NAMES]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import singlespmv_amd as sp  # noqa: E402

ALPHA, BETA = -2.5, 0.75
SWITCH = "SPMV_LAUNCH_AXPBY_GENERIC"


def matrices(scale):
    m = int(2_000_000 * scale)
    yield "banded64", m, lambda: sp.generate_csr(sp.gen_spec("banded", m, band_lo=-32, band_hi=31, seed=4)), \
        ("dia", "ell", "csr")
    m2 = int(10_000_000 * scale)
    yield "uniform16", m2, lambda: sp.generate_csr(sp.gen_spec("uniform", m2, per_row=16, seed=2)), ("csr", "ell", "bin")
    m3 = int(5_000_000 * scale)
    yield "powerlaw", m3, lambda: sp.generate_csr(sp.gen_spec("powerlaw", m3, max_len=10000, alpha=2.0, seed=3)), \
        ("csr", "bin")


def time_plan(plan, m, rounds, iters, probes):
    """min ms per call of execute, axpby (the plan's path) and the forced generic route."""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    y = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    best = {"execute": float("inf"), "axpby": float("inf"), "generic": float("inf") if probes else None}

    def run(variant, n):
        # y is updated in place n times; |beta| < 1, so it stays bounded
        if variant == "execute":
            return plan.time(x, y, n) / n
        y.uniform_(generator=g)
        if variant == "generic":
            os.environ[SWITCH] = "1"
        try:
            return plan.time_axpby(x, y, ALPHA, BETA, n) / n
        finally:
            os.environ.pop(SWITCH, None)

    for r in range(rounds + 1):  # round 0: warm-up (code objects loaded, scratch allocated)
        for variant in best:
            if best[variant] is None:
                continue
            ms = run(variant, iters if r else 1)
            if r:
                best[variant] = min(best[variant], ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = the sizes above)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    a = ap.parse_args()
    probes = "probes" in os.environ.get("SPMV_HIP_LIBRARY", "")
    out = open(a.out, "a") if a.out else sys.stdout
    for name, m, gen, fmts in matrices(a.scale):
        if a.only and name not in a.only.split(","):
            continue
        rp, col, val = gen()
        for fmt in fmts:
            plan = sp.Plan.from_csr(m, m, rp, col, val, fmt)
            info = plan.info()
            path = plan.axpby_path()
            best = time_plan(plan, m, a.rounds, a.iters, probes)
            b0 = info["algo_bytes"]
            model = {"execute": b0, "axpby": b0 + (8 if path == "fused" else 32) * m, "generic": b0 + 32 * m}
            rec = {"matrix": name, "m": m, "nnz": int(rp[-1]), "format": info["format"], "kernel": info["kernel"],
                   "path": path, "alpha": ALPHA, "beta": BETA, "probe_build": probes,
                   "bytes_execute": b0, "bytes_fused": b0 + 8 * m, "bytes_generic": b0 + 32 * m,
                   "rounds": a.rounds, "iters": a.iters}
            for v, ms in best.items():
                rec[f"ms_{v}"] = None if ms is None else round(ms, 5)
                rec[f"gbs_{v}"] = None if ms is None else round(model[v] / ms / 1e6, 1)
            if best["generic"] is not None:
                rec["axpby_vs_generic"] = round(best["axpby"] / best["generic"], 4)
            rec["axpby_vs_execute"] = round(best["axpby"] / best["execute"], 4)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            plan.destroy()
            torch.cuda.empty_cache()
        del rp, col, val
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
