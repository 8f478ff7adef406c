#!/usr/bin/env python3
"""Plan.cg (spmv_cg_solve) against the same iteration composed from the public
API a caller had before it.

For each (matrix, format) one plan is built; in ONE process, on that plan,
device buffers throughout, a solve of `iters` iterations (rtol = 0, so every
iteration runs) is timed on the wall clock between two device
synchronisations, for these variants:

  cg_e8, cg_e64              plan.cg(check_every = 8 / 64)
  cg_graph_e8, cg_graph_e64  the same with graph=True (the graph is cached on
                             the plan: the warm-up round pays its capture)
  yardstick_dev   (a) plan.execute_dot(p, q, w=p, dots on the device, async) and
                  torch vector operations, alpha and beta as 0-dim device
                  tensors: no host look at all during the solve
  yardstick_item  (b) the same with .item() for p . Ap and r . z every step
  dot             plan.time_dot(p, q, p): the SpMV with its dot alone, per call

THE yardsticks are (a) and (b): what a caller writes without the solver, never
the new code itself.  Both run the recurrences of include/spmv_hip.h (they
need not agree bit for bit: torch.dot adds in its own order).  Rounds are
interleaved (every variant once per round) and the minimum per variant is
kept, the spread (max / min) recorded; compare only within one process and one
plan (placements move a kernel by up to ~10 %).

One JSON line per (matrix, format): us_* = microseconds per iteration (min),
spread_*, launches = spmv_cg_path, vector_share = 1 - us_dot / us_cg_e64
(what update, finish and direction add beside the SpMV and its dot), and
cg_vs_dev = us_cg_e64 / us_yardstick_dev, cg_graph_vs_dev likewise (below 1:
the solve is faster).

Matrices (symmetric M-matrices: off-diagonals -1, diagonal = their count +
0.01, so 200 iterations neither converge to an exact zero nor break down):
  uniform16  16 off-diagonals per row at 8 seeded strides, both ways (rows
             wrap): bin, ell
  banded64   64 off-diagonals (offsets +-1 .. +-32) and the main diagonal: dia, csr

  python tools/cg_times.py [--out FILE] [--scale 1.0] [--rounds 5] [--iters 200] [--only NAMES]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import singlespmv_amd as sp  # noqa: E402

SHIFT = 0.01


def uniform16(m):
    rng = np.random.default_rng(21)
    strides = rng.choice(np.arange(1, m // 2), 8, replace=False)
    offs = np.concatenate([[0], strides, -strides]).astype(np.int64)
    col = np.sort((np.arange(m, dtype=np.int64)[:, None] + offs[None, :]) % m, axis=1)
    val = np.where(col == np.arange(m)[:, None], 16.0 + SHIFT, -1.0)
    return np.arange(m + 1, dtype=np.int64) * 17, col.astype(np.int32).ravel(), val.ravel()


def banded64(m):
    offs = np.arange(-32, 33, dtype=np.int64)
    col = np.arange(m, dtype=np.int64)[:, None] + offs[None, :]
    ok = (col >= 0) & (col < m)
    count = ok.sum(axis=1)
    val = np.where(offs[None, :] == 0, (count - 1 + SHIFT)[:, None], -1.0)
    rp = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    return rp, col[ok].astype(np.int32), np.ascontiguousarray(val[ok])


def matrices(scale):
    m = int(2_000_000 * scale) | 1  # odd: the vector kernels' last row too
    yield "uniform16", m, lambda: uniform16(m), ("bin", "ell")
    yield "banded64", m, lambda: banded64(m), ("dia", "csr")


def composed(plan, b, x, dinv, iters, item):
    """Yardsticks (a) and (b): the iteration of spmv_cg_solve from execute_axpby,
    execute_dot and torch."""
    m = b.numel()
    dots = torch.zeros(2, dtype=torch.float64, device="cuda")
    q = torch.empty(m, dtype=torch.float64, device="cuda")
    r = b.clone()
    plan.execute_axpby(x, r, alpha=-1.0, beta=1.0, async_=True)
    z = dinv * r
    p = z.clone()
    rz = torch.dot(r, z)
    if item:
        rz = rz.item()
    for _ in range(iters):
        plan.execute_dot(p, q, p, dots=dots, async_=True)
        alpha = rz / (dots[0].item() if item else dots[0])
        if item:
            x.add_(p, alpha=alpha)
            r.sub_(q, alpha=alpha)
        else:
            x.addcmul_(p, alpha)
            r.addcmul_(q, -alpha)
        torch.mul(dinv, r, out=z)
        rz_new = torch.dot(r, z)
        torch.dot(r, r)  # rr, the stopping test's
        if item:
            rz_new = rz_new.item()
        beta = rz_new / rz
        rz = rz_new
        p.mul_(beta).add_(z)
    return x


def time_plan(plan, m, diag, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    b = torch.rand(m, dtype=torch.float64, device="cuda", generator=g)
    dinv = (1.0 / torch.from_numpy(diag)).cuda()
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    dots = torch.zeros(2, dtype=torch.float64, device="cuda")
    q = torch.zeros(m, dtype=torch.float64, device="cuda")
    last = {}

    def wall(body):
        x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        body()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / iters

    def cg(every, graph):
        def run():
            last["info"] = plan.cg(b, x, dinv, rtol=0.0, max_iters=iters, check_every=every, graph=graph)
        return run

    variants = {"cg_e8": cg(8, False), "cg_e64": cg(64, False), "cg_graph_e8": cg(8, True), "cg_graph_e64": cg(64, True),
                "yardstick_dev": lambda: composed(plan, b, x, dinv, iters, False),
                "yardstick_item": lambda: composed(plan, b, x, dinv, iters, True)}
    seen = {v: [] for v in variants}
    seen["dot"] = []
    for r in range(rounds + 1):  # round 0: warm-up (workspace, graphs, code objects)
        for v, run in variants.items():
            us = wall(run)
            if v.startswith("cg"):
                info = last["info"]
                assert info["status"] == "max_iters" and info["iterations"] == iters, (v, info)
            if r:
                seen[v].append(us)
        us = plan.time_dot(b, q, b, dots, 20) / 20 * 1e3
        if r:
            seen["dot"].append(us)
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = 2 M rows)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else sys.stdout
    for name, m, gen, fmts in matrices(a.scale):
        if a.only and name not in a.only.split(","):
            continue
        rp, col, val = gen()
        diag = val[col == np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))]
        for fmt in fmts:
            plan = sp.Plan.from_csr(m, m, rp, col, val, fmt)
            info = plan.info()
            seen = time_plan(plan, m, diag, a.rounds, a.iters)
            rec = {"matrix": name, "m": m, "nnz": int(rp[-1]), "format": info["format"], "kernel": info["kernel"],
                   "dot_path": plan.dot_path(), "launches": plan.cg_path(), "rounds": a.rounds, "iters": a.iters}
            for v, us in seen.items():
                rec[f"us_{v}"] = round(min(us), 2)
                rec[f"spread_{v}"] = round(max(us) / min(us), 3)
            rec["vector_share"] = round(1.0 - min(seen["dot"]) / min(seen["cg_e64"]), 4)
            rec["cg_vs_dev"] = round(min(seen["cg_e64"]) / min(seen["yardstick_dev"]), 4)
            rec["cg_graph_vs_dev"] = round(min(seen["cg_graph_e64"]) / min(seen["yardstick_dev"]), 4)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            plan.destroy()
            torch.cuda.empty_cache()
        del rp, col, val
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
