"""CPU figures for profiles/wide_routes_model_error.txt: for the inputs of every case of tests/test_gpu_wide_routes.py, the error
of a NumPy restatement of the scaled bodies' arithmetic (tests/wide_routes.py: scaled_model — f16(d sc q) x f16(d8 code 2^-e), the
mins as f16(-dmin m) x f16(d8 bsum 2^-e), f64 sums) against the oracle on the Q8_K-quantised activations.  The project's bounds
for these bodies (normwise 1e-3, no element beyond 1.5e-3 (|G| + rms)) were measured at k = 4096 / 14336; this says what the
arithmetic alone costs at k = 256 .. 1024, before any GPU runs.  A case whose model error exceeds half a bound needs other inputs.

    python tools/wide_routes_model_error.py            # prints one line per case and matrix; needs no GPU"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llamafile_amd import ggml_types as T  # noqa: E402
from oracle import ora  # noqa: E402
import wide_routes as R  # noqa: E402


def line(tag, t, m, n, k, raw, x, B):
    ok, G = ora.sgemm(t, raw, T.Q8_K, B, m, n, k, nth=8)
    assert ok == 1
    err, frac, worst = R.figures(R.scaled_model(t, raw, k, x, B), G)
    flag = "" if err <= R.SCALED_TOL / 2 and worst <= R.ELEM_RTOL / 2 else "  ** above half a bound **"
    print(f"WIDE_ROUTE_MODEL {tag} {T.NAMES[t]} m={m} n={n} k={k}: normwise={err:.3e} frac_over_1.5e-3={frac:.4f} worst_elem={worst:.3e}{flag}",
          flush=True)


def main():
    ora.build()
    for r in R.RUNS:
        name, t, control = r
        _, _, ms, n, nb, _ = R.CASES[name]
        raws, x, B = R.inputs(ms, t, n, nb * 256, R.seed_of(name), control)
        for j, (m, raw) in enumerate(zip(ms, raws)):
            line(f"{R.run_id(r)}[{j}]", t, m, n, nb * 256, raw, x, B)
    _, t, ms, n, nb = R.KR_STAGED
    raws, x, B = R.inputs(ms, t, n, nb * 256, R.seed_of("kr-staged"))
    for j, (m, raw) in enumerate(zip(ms, raws)):
        line(f"kr-staged[{j}]", t, m, n, nb * 256, raw, x, B)
    pairs, ms, n, nb = R.DUAL
    for ts in pairs:
        raws, x, B = R.inputs(ms, ts, n, nb * 256, R.seed_of("dual"))
        for j, (m, raw) in enumerate(zip(ms, raws)):
            line(f"dual-{T.NAMES[ts[0]]}+{T.NAMES[ts[1]]}[{j}]", ts[j], m, n, nb * 256, raw, x, B)


if __name__ == "__main__":
    main()
