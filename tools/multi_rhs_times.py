#!/usr/bin/env python3
"""Multi-vector execute against single-vector executes, on the same plans.

For each (matrix, format) one plan is built; in ONE process, on that plan,
spmv_time_multi is timed for k = 1, 2, 4, 8 and 13 interleaved columns beside
spmv_time for one contiguous vector.  Rounds are interleaved (every variant
once per round, so drift and neighbours hit all of them alike) and the
minimum per variant is kept.  The yardstick of a fused width K is K
single-vector executes on the same plan: compare only within one process and
one plan, never across runs (placements move a kernel by up to ~10 %,
DESIGN §3.6).

One JSON line per (matrix, format, k):
  ms_multi      one multi execute of k columns (min over rounds)
  ms_single     one spmv_time execute of a contiguous vector, same plan
  vs_k_singles  ms_multi / (k * ms_single): < 1 = the multi call wins
  path          spmv_multi_path's width list

Matrices:
  banded64   64 diagonals, 2 M rows (1 GB of DIA values): dia, ell
  uniform16  16 per row, 10 M x 10 M (config 2): ell (fused), bin, csr (generic)
  tri1500    diagonals -1500, 0, 1500, 4 M rows: dia -- the x window fits the
             LDS at K = 2 and 4, not at 8 (global-x kernel)

--dia-variants (probe build only: make probes, SPMV_HIP_LIBRARY=
probes_build/libspmv_hip.so) also times every fused DIA width with the x
window staged in LDS and with x read from global memory, on the same plan
(SPMV_LAUNCH_DIA_MULTI_LDSX, read at every launch): "variant" ldsx / globalx,
and ldsx-cap96 = staged with the 96-KB LDS request that caps the single-vector
launch of a large plan at one workgroup per CU (SPMV_LAUNCH_DIA_MULTI_LDS_KB=96).

  python tools/multi_rhs_times.py [--out FILE] [--scale 1.0] [--rounds 7] [--iters 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import singlespmv_amd as sp  # noqa: E402

KS = (1, 2, 4, 8, 13)


def tridiag(m, d):
    r = np.repeat(np.arange(m, dtype=np.int64), 3)
    c = r + np.tile(np.array([-d, 0, d], np.int64), m)
    keep = (c >= 0) & (c < m)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=m))]).astype(np.int64)
    rng = np.random.default_rng(7)
    return rp, c[keep].astype(np.int32), rng.uniform(0.5, 1.0, int(rp[-1]))


def matrices(scale):
    m = int(2_000_000 * scale)
    yield "banded64", m, lambda: sp.generate_csr(sp.gen_spec("banded", m, band_lo=-32, band_hi=31, seed=4)), ("dia", "ell")
    m2 = int(10_000_000 * scale)
    yield "uniform16", m2, lambda: sp.generate_csr(sp.gen_spec("uniform", m2, per_row=16, seed=2)), ("ell", "bin", "csr")
    m3 = int(4_000_000 * scale)
    yield "tri1500", m3, lambda: tridiag(m3, 1500), ("dia",)


def time_plan(plan, m, rounds, iters):
    """{k: min ms per call} for the multi variants, and the single-vector min."""
    g = torch.Generator(device="cuda").manual_seed(1)
    blocks = {}
    for k in KS:
        ld = k + (k & 1)  # even row stride: the fused path's condition
        X = torch.rand((m, ld), dtype=torch.float64, device="cuda", generator=g)
        Y = torch.empty((m, ld), dtype=torch.float64, device="cuda")
        blocks[k] = (X[:, :k], Y[:, :k], ld)
    x = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    y = torch.empty(m, dtype=torch.float64, device="cuda")
    plan.time(x, y, 2)  # warm-up: code objects loaded, scratch allocated
    for k in KS:
        plan.time_multi(blocks[k][0], blocks[k][1], 1)
    best = {k: float("inf") for k in KS}
    single = float("inf")
    for _ in range(rounds):
        single = min(single, plan.time(x, y, iters) / iters)
        for k in KS:
            best[k] = min(best[k], plan.time_multi(blocks[k][0], blocks[k][1], iters) / iters)
    paths = {k: plan.multi_path(blocks[k][0], blocks[k][1]) for k in KS}
    return best, single, paths, {k: blocks[k][2] for k in KS}


def time_dia_variants(plan, m, rounds, iters):
    """{(K, variant): min ms}: the fused DIA widths with LDS staging forced on (where it fits) and off."""
    g = torch.Generator(device="cuda").manual_seed(1)
    best = {}
    blocks = {}
    for k in (2, 4, 8):
        X = torch.rand((m, k), dtype=torch.float64, device="cuda", generator=g)
        blocks[k] = (X, torch.empty((m, k), dtype=torch.float64, device="cuda"))
        for v in ("globalx", "ldsx"):
            best[(k, v)] = float("inf")
        best[(k, "ldsx-cap96")] = float("inf")
    # ldsx-cap96: LDS-staged with launch_dia's 96-KB LDS request (one workgroup per CU)
    variants = (("globalx", "0", None), ("ldsx", "1", None), ("ldsx-cap96", "1", "96"))
    try:
        for r in range(rounds + 1):  # round 0: warm-up
            for k in (2, 4, 8):
                for v, e, kb in variants:
                    os.environ["SPMV_LAUNCH_DIA_MULTI_LDSX"] = e
                    os.environ.pop("SPMV_LAUNCH_DIA_MULTI_LDS_KB", None)
                    if kb is not None:
                        os.environ["SPMV_LAUNCH_DIA_MULTI_LDS_KB"] = kb
                    ms = plan.time_multi(blocks[k][0], blocks[k][1], iters) / iters
                    if r:
                        best[(k, v)] = min(best[(k, v)], ms)
    finally:
        os.environ.pop("SPMV_LAUNCH_DIA_MULTI_LDSX", None)
        os.environ.pop("SPMV_LAUNCH_DIA_MULTI_LDS_KB", None)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = the sizes above)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    ap.add_argument("--dia-variants", action="store_true", help="probe build: LDS-staged against global x per DIA width")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    for name, m, gen, fmts in matrices(a.scale):
        if a.only and name not in a.only.split(","):
            continue
        rp, col, val = gen()
        for fmt in fmts:
            plan = sp.Plan.from_csr(m, m, rp, col, val, fmt)
            info = plan.info()
            best, single, paths, lds = time_plan(plan, m, a.rounds, a.iters)
            for k in KS:
                rec = {"matrix": name, "m": m, "nnz": int(rp[-1]), "format": info["format"], "kernel": info["kernel"],
                       "k": k, "ld": lds[k], "path": paths[k], "ms_multi": round(best[k], 5),
                       "ms_single": round(single, 5), "vs_k_singles": round(best[k] / (k * single), 4),
                       "rounds": a.rounds, "iters": a.iters}
                out.write(json.dumps(rec) + "\n")
                out.flush()
            if a.dia_variants and info["format"] == "dia":
                if "probes" not in os.environ.get("SPMV_HIP_LIBRARY", ""):
                    raise SystemExit("--dia-variants needs the probe build (SPMV_HIP_LIBRARY=probes_build/libspmv_hip.so)")
                for (k, v), ms in sorted(time_dia_variants(plan, m, a.rounds, a.iters).items()):
                    rec = {"matrix": name, "m": m, "format": "dia", "n_diags": info["n_diags"], "k": k, "variant": v,
                           "ms_multi": round(ms, 5), "ms_single": round(single, 5),
                           "vs_k_singles": round(ms / (k * single), 4), "rounds": a.rounds, "iters": a.iters}
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
            plan.destroy()
            torch.cuda.empty_cache()
        del rp, col, val
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
