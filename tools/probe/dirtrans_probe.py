#!/usr/bin/env python3
"""Times the direct transform at TL1279 -> O1280 / 137 fields (device arrays, the object's stream) against the inverse transform
of the same object, with the per-stage HIP-event times of both (profile=1).  One JSON line per block of calls, written to stdout
and to the file given as the first argument (e.g. profiles/r07_dirtrans_probe.jsonl).

    python tools/probe/dirtrans_probe.py [out.jsonl] [--grid O1280] [--T 1279] [--nf 137] [--steps 10] [--blocks 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--grid", default="O1280")
    ap.add_argument("--T", type=int, default=1279)
    ap.add_argument("--nf", type=int, default=137)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    import torch
    import atlas_amd
    g = atlas_amd.Grid(a.grid)
    tr = atlas_amd.Trans(g, a.T, dirtrans=1)
    npts, ncoef = g.size(), tr.nb_spectral_coefficients()
    gen = torch.Generator(device="cuda").manual_seed(1)
    gp = torch.randn(a.nf * npts, dtype=torch.float64, device="cuda", generator=gen)
    sp = torch.zeros(a.nf * ncoef, dtype=torch.float64, device="cuda")
    tr.use_torch_stream()
    for _ in range(2):                      # first calls: buffers, warm-up
        tr.dirtrans(a.nf, gp, sp)
        tr.invtrans(a.nf, sp, gp)
    torch.cuda.synchronize()
    lines = []
    for blk in range(a.blocks):
        row = {"grid": a.grid, "T": a.T, "nf": a.nf, "steps": a.steps, "block": blk}
        for name, call in (("dirtrans", lambda: tr.dirtrans(a.nf, gp, sp)), ("invtrans", lambda: tr.invtrans(a.nf, sp, gp))):
            tr.set_profile(False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            torch.cuda.synchronize()
            row[f"{name}_ms"] = (time.perf_counter() - t0) * 1e3 / a.steps
        tr.set_profile(True)
        tr.timings(reset=True)
        tr.timings_dirtrans(reset=True)
        for _ in range(a.steps):
            tr.dirtrans(a.nf, gp, sp)
            tr.invtrans(a.nf, sp, gp)
        td, ti = tr.timings_dirtrans(reset=True), tr.timings(reset=True)
        row["dir_fourier_ms"] = td["fourier_ms"] / max(td["fourier_calls"], 1)
        row["dir_legendre_ms"] = td["legendre_ms"] / max(td["legendre_calls"], 1)
        row["inv_legendre_ms"] = ti["legendre_ms"] / max(ti["legendre_calls"], 1)
        row["inv_fourier_ms"] = ti["fourier_ms"] / max(ti["fourier_calls"], 1)
        row["legendre_gflop"] = tr.legendre_flops(a.nf) / 1e9
        print(json.dumps(row), flush=True)
        lines.append(row)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
