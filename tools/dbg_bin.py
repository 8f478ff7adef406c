# Reproduce test_bin_layout_knobs in one process: every knob, several plans,
# repeated executes; report executes whose y differs from the oracle.  The
# padding and the Sum waves are plan options; SPMV_BIN_REUSE and SPMV_BIN_DEBUG
# are probe-build switches (SPMV_HIP_LIBRARY=probes_build/libspmv_hip.so; the
# product library ignores them).  Ends with one JSON line.
import json, os, sys, numpy as np
sys.path.insert(0, os.getcwd())
import singlespmv_amd as sp, oracle
m = 120_000
spec = sp.gen_spec("powerlaw", m, m, per_row=11, max_len=5000, seed=41)
rp, col, val = sp.generate_csr(spec)
x = sp.generate_vector(m, seed=43)
yo = oracle.csr_spmv(rp, col, val, x)
# (plan options, probe-build environment)
knobs = [({"bin_pad": 8}, {}), ({"bin_pad": 32}, {}), ({"bin_sum_waves": 2}, {}), ({"bin_sum_waves": 8}, {}),
         ({}, {"SPMV_BIN_REUSE": "1"}), ({}, {"SPMV_BIN_DEBUG": "1"}), ({}, {})]
plans = bad_executes = 0
for rnd in range(3):
    for opts, env in knobs:
        for k in ("SPMV_BIN_REUSE", "SPMV_BIN_DEBUG"):
            os.environ.pop(k, None)
        os.environ.update(env)
        p = sp.Plan.from_csr(m, m, rp, col, val, "bin", bin_groups=2, **opts)
        out = []
        for rep in range(20):
            y = np.full(m, 1.2345e300 * (-1) ** rep)
            p.execute(x, y)
            bad = np.flatnonzero(y != yo)
            if len(bad):
                out.append((rep, len(bad), bad[:4].tolist(), (y[bad[:2]] - yo[bad[:2]]).tolist()))
        print(rnd, opts, env, "bad executes:", out[:5], flush=True)
        plans += 1
        bad_executes += len(out)
        p.destroy()
print(json.dumps({"tool": "dbg_bin", "library": os.environ.get("SPMV_HIP_LIBRARY", ""), "rows": m, "plans": plans,
                  "executes": plans * 20, "bad_executes": bad_executes}), flush=True)
