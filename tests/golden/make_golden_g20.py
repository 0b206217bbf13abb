"""Golden G20: the engine-call traces of the host samplers (tests/test_sampler_trace_cpu.py holds the harness and the cases).

    python tests/golden/make_golden_g20.py             regenerate g20_sampler_traces.json, keeping the commit hash it names
    python tests/golden/make_golden_g20.py --record    record anew from HEAD: refused unless diff_foley_amd/ is HEAD's, unmodified

No device and no reference checkout: the yardstick is this package at the recorded commit.  The samplers are reached through
diff_foley_amd.DDIMSampler / PLMSSampler / DPMSolverSampler, LatentDiffusion.sample and LatentDiffusion.dpm_solver only, so the
maker runs unchanged on either side of a rewrite of the host layer, and on the same behaviour it writes the same bytes.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_sampler_trace_cpu as T  # noqa: E402


def _git(*args):
    return subprocess.run(("git", "-C", ROOT) + args, check=True, capture_output=True, text=True).stdout.strip()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="take HEAD as the new yardstick")
    args = ap.parse_args()
    if args.record:
        if _git("status", "--porcelain", "--", "diff_foley_amd"):
            raise SystemExit("diff_foley_amd/ differs from HEAD: a recording names the commit whose behaviour it holds")
        commit = _git("rev-parse", "HEAD")
    else:
        with open(T.FIXTURE) as f:
            commit = json.load(f)["commit"]
    text = T.render(T.all_traces(), commit)
    with open(T.FIXTURE, "w") as f:
        f.write(text)
    print(f"{T.FIXTURE}: {len(T.CASES)} cases, {sum(len(v) for v in T.all_traces().values())} calls, {len(text)} bytes, commit {commit}")
