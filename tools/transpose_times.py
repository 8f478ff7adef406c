#!/usr/bin/env python3
"""The transposition (spmv_csr_transpose_device, Plan.from_device_csr with
transpose=True) against what a device-resident caller does without it: the CSR
to the host, spmv_csr_transpose there (a stable counting sort on one core),
the result back to the device, then an ordinary Plan.from_device_csr.

One child process per matrix, each under its own `timeout`; the first child
that fails ends the run (nothing is retried, nothing more is started on the
device).  In a child, after one warm-up of each, --rounds interleaved rounds
of the three device measurements, minimum of each (wall clock around the
call, device synchronised):

  ms_transpose_device   csr_transpose on device tensors, values and no perm
  ms_build_transposed   Plan.from_device_csr(A, transpose=True)
  ms_build_companion    Plan.from_device_csr of the pre-transposed CSR, same
                        format; transpose_cost = the difference
and once each:
  ms_transpose_host     csr_transpose on the host arrays (min of --host-reps)
  ms_d2h, ms_h2d        A's three arrays to the host, A^T's three back
  floor_ms              read 12 nnz + 8 (m + 1) at the measured read stream
                        rate + write 12 nnz + 8 (n + 1) at the measured write
                        stream rate (spmv_stream_probe, spmv_stream_write_probe)
  over_floor            ms_transpose_device / floor_ms
  host_path_ms          ms_d2h + ms_transpose_host + ms_h2d: the yardstick
  digests_equal         the two plans are the same arrays (spmv_plan_digest)

Matrices:
  uniform16  10 M x 10 M, 16 per row (config 2): bin
  powerlaw   5 M power-law rows (config 3): bin
  banded64   64 diagonals x 2 M rows: dia

  python tools/transpose_times.py [--out FILE] [--scale 1.0] [--only NAMES] [--timeout 560]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRICES = [("uniform16", "bin"), ("powerlaw", "bin"), ("banded64", "dia")]


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


def child(name, fmt, a):
    import torch

    import singlespmv_amd as sp

    m, rp, col, val = generate(sp, name, a.scale)
    n, nnz = m, int(rp[-1])

    def wall(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t) * 1e3

    ms_host = float("inf")
    for _ in range(a.host_reps):
        t, ms = wall(lambda: sp.csr_transpose(m, n, rp, col, val))
        ms_host = min(ms_host, ms)
    drp, dcol, dval = (torch.from_numpy(x).cuda() for x in (rp, col, val))
    _, ms_d2h = wall(lambda: [x.cpu() for x in (drp, dcol, dval)])
    dt, ms_h2d = wall(lambda: [torch.from_numpy(x).cuda() for x in t])
    del rp, col, val

    def transpose():
        return wall(lambda: sp.csr_transpose(m, n, drp, dcol, dval))

    def build_t():
        return wall(lambda: sp.Plan.from_device_csr(m, n, drp, dcol, dval, fmt, transpose=True))

    def build_c():
        return wall(lambda: sp.Plan.from_device_csr(n, m, dt[0], dt[1], dt[2], fmt))

    got, _ = transpose()  # warm-ups: code objects loaded
    same_bytes = all(bool((g.view(torch.int64) == w.view(torch.int64)).all()) if g.dtype == torch.float64
                     else bool((g == w).all()) for g, w in zip(got, dt))
    del got
    pt, _ = build_t()
    pc, _ = build_c()
    info = pt.info()
    digests_equal = pt.digest() == pc.digest()
    pt.destroy()
    pc.destroy()
    best = {"t": float("inf"), "bt": float("inf"), "bc": float("inf")}
    for _ in range(a.rounds):
        for key, f in (("t", transpose), ("bt", build_t), ("bc", build_c)):
            r, ms = f()
            best[key] = min(best[key], ms)
            if key != "t":
                r.destroy()
            del r
    read_gbs = sp.stream_probe(0, 2 << 30, 10)
    write_gbs = sp.stream_write_probe(0, 2 << 30, 10)
    floor_ms = (12 * nnz + 8 * (m + 1)) / read_gbs / 1e6 + (12 * nnz + 8 * (n + 1)) / write_gbs / 1e6
    rec = {"matrix": name, "m": m, "n": n, "nnz": nnz, "format": info["format"], "kernel": info["kernel"],
           "ms_transpose_device": round(best["t"], 3), "ms_build_transposed": round(best["bt"], 3),
           "ms_build_companion": round(best["bc"], 3), "transpose_cost": round(best["bt"] - best["bc"], 3),
           "ms_transpose_host": round(ms_host, 3), "ms_d2h": round(ms_d2h, 3), "ms_h2d": round(ms_h2d, 3),
           "host_path_ms": round(ms_d2h + ms_host + ms_h2d, 3),
           "host_path_over_device": round((ms_d2h + ms_host + ms_h2d) / best["t"], 1),
           "host_over_device": round(ms_host / best["t"], 1),
           "read_gbs": round(read_gbs, 1), "write_gbs": round(write_gbs, 1), "floor_ms": round(floor_ms, 3),
           "over_floor": round(best["t"] / floor_ms, 2), "same_bytes_as_host": same_bytes,
           "digests_equal": digests_equal, "rounds": a.rounds, "host_reps": a.host_reps}
    print(json.dumps(rec), flush=True)
    return 0 if same_bytes and digests_equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (1.0 = the sizes above)")
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=560, help="seconds per child process")
    ap.add_argument("--one", default="", help="(internal) matrix:format of this child")
    a = ap.parse_args()
    if a.one:
        name, fmt = a.one.split(":")
        return child(name, fmt, a)
    want = set(a.only.split(",")) if a.only else None
    out = open(a.out, "a") if a.out else sys.stdout
    for name, fmt in MATRICES:
        if want and name not in want:
            continue
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one",
               f"{name}:{fmt}", "--scale", str(a.scale), "--rounds", str(a.rounds), "--host-reps", str(a.host_reps)]
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
