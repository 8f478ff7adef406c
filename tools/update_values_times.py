#!/usr/bin/env python3
"""Value refresh (Plan.prepare_update / Plan.update_values) against what a
user does without it: a fresh Plan.from_device_csr with the same options.

One child process per plan, each under its own `timeout`; the first child
that fails ends the run (nothing is retried, nothing more is started on the
device).  In a child, on ONE plan built from device tensors:

  ms_rebuild   a fresh Plan.from_device_csr, same options (wall clock around
               the call, device synchronised; min of --rebuilds after one
               warm-up build) -- the yardstick, existing code
  ms_prepare   prepare_update, once (wall clock, device synchronised)
  ms_update    a device-resident update_values: events on the plan's stream,
               min of --updates after a warm-up, alternating two value sets
  ms_execute   one spmv_time execute on the same plan
  model_bytes  the update's traffic: 4 B map + 8 B store per value slot
               (8 B map from 2^31 - 1 entries), + 8 B read per entry
  model_gbs    model_bytes / ms_update; frac_stream = model_gbs / the
               device's measured mixed read+write stream rate (spmv_mixed_probe,
               2/4 written back), measured once per child

Plans:
  banded64   64 diagonals x 2 M rows: dia, ell, csr
  uniform16  10 M x 10 M, 16 per row (config 2): bin, ell, csr
  powerlaw   5 M power-law rows: bin

  python tools/update_values_times.py [--out FILE] [--scale 1.0] [--only NAMES] [--timeout 420]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANS = [("banded64", "dia"), ("banded64", "ell"), ("banded64", "csr"),
         ("uniform16", "bin"), ("uniform16", "ell"), ("uniform16", "csr"),
         ("powerlaw", "bin")]


def generate(sp, name, scale):
    if name == "banded64":
        m = int(2_000_000 * scale)
        return (m,) + sp.generate_csr(sp.gen_spec("banded", m, band_lo=-32, band_hi=31, seed=4))
    if name == "uniform16":
        m = int(10_000_000 * scale)
        return (m,) + sp.generate_csr(sp.gen_spec("uniform", m, per_row=16, seed=2))
    if name == "powerlaw":
        m = int(5_000_000 * scale)
        return (m,) + sp.generate_csr(sp.gen_spec("powerlaw", m, max_len=10000, seed=3))
    raise SystemExit(f"unknown matrix {name}")


def value_slots(info, nnz):
    """Value slots of the plan's layout (include/spmv_hip.h)."""
    f = info["format"]
    if f == "csr":
        return (nnz if info["csr_lanes"] == 0 else (nnz + 255) // 256 * 256) + 8
    if f in ("hyb", "jds"):
        return info["stored_slots"] + 8
    if f == "bin":
        return info["stored_slots"] + 512
    return info["stored_slots"]


def child(name, fmt, a):
    import numpy as np
    import torch

    import singlespmv_amd as sp

    m, rp, col, val = generate(sp, name, a.scale)
    nnz = int(rp[-1])
    drp, dcol, dv0 = (torch.from_numpy(t).cuda() for t in (rp, col, val))
    dv1 = dv0 * -1.5 + 0.25
    del rp, col, val
    x = torch.rand(m, dtype=torch.float64, device="cuda")
    y = torch.empty(m, dtype=torch.float64, device="cuda")

    def build():
        torch.cuda.synchronize()
        t = time.perf_counter()
        p = sp.Plan.from_device_csr(m, m, drp, dcol, dv0, fmt)
        torch.cuda.synchronize()
        return p, (time.perf_counter() - t) * 1e3

    plan, first = build()
    rebuilds = []
    for _ in range(a.rebuilds):
        q, ms = build()
        rebuilds.append(ms)
        q.destroy()
    info = plan.info()
    torch.cuda.synchronize()
    t = time.perf_counter()
    plan.prepare_update(drp, dcol)
    torch.cuda.synchronize()
    ms_prepare = (time.perf_counter() - t) * 1e3
    sets = (dv1, dv0)
    plan.update_values(dv1)  # warm-up: code object loaded
    plan.update_values(dv0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms_update = float("inf")
    for i in range(a.updates):  # the plan runs on the null stream, torch's default
        e0.record()
        plan.update_values(sets[i & 1], async_=True)
        e1.record()
        e1.synchronize()
        ms_update = min(ms_update, e0.elapsed_time(e1))
    plan.time(x, y, 2)
    ms_execute = min(plan.time(x, y, 5) / 5 for _ in range(5))
    slots = value_slots(info, nnz)
    model = (8 if nnz >= 2 ** 31 - 1 else 4) * slots + 8 * slots + 8 * nnz
    stream = sp.mixed_probe(0, 1792 << 20, 2, 10)
    rec = {"matrix": name, "m": m, "nnz": nnz, "format": info["format"], "kernel": info["kernel"],
           "value_slots": slots, "ms_first_build": round(first, 3), "ms_rebuild": round(min(rebuilds), 3),
           "ms_prepare": round(ms_prepare, 3), "ms_update": round(ms_update, 4), "ms_execute": round(ms_execute, 4),
           "rebuild_over_update": round(min(rebuilds) / ms_update, 1), "model_bytes": model,
           "model_gbs": round(model / ms_update / 1e6, 1), "stream_gbs": round(stream, 1),
           "frac_stream": round(model / ms_update / 1e6 / stream, 3), "updates": a.updates, "rebuilds": a.rebuilds}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = the sizes above)")
    ap.add_argument("--only", default="", help="comma-separated matrix:format pairs or matrix names")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--rebuilds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    ap.add_argument("--one", default="", help="(internal) matrix:format of this child")
    a = ap.parse_args()
    if a.one:
        name, fmt = a.one.split(":")
        child(name, fmt, a)
        return 0
    want = set(a.only.split(",")) if a.only else None
    out = open(a.out, "a") if a.out else sys.stdout
    for name, fmt in PLANS:
        if want and name not in want and f"{name}:{fmt}" not in want:
            continue
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one",
               f"{name}:{fmt}", "--scale", str(a.scale), "--updates", str(a.updates), "--rebuilds", str(a.rebuilds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                out.write(line + "\n")
                out.flush()
        if r.returncode != 0:  # a failed child: nothing more runs on the device
            print(f"{name}:{fmt} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    if a.out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
