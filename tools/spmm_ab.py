#!/usr/bin/env python3
"""MatMatMult against k MatMults on one handle, in one process:
the 7-point Poisson operand assembled on the device, on its row-template plan
(path 2) and with row_templates = row_patterns = column_codes = 0 (path 1,
CSR row blocks), both dense layouts, k in {2, 4, 8}. For each case the arms —
mat_mult, the k mults of the columns, and with --pair mat_mult's 16-byte pair
variant (AIJHIP_SPMM_PAIR; interleaved only) — are warmed up, checked bit for
bit against each other at the timed size, then timed in turn, round after
round, with HIP events around every launch. One JSON line per case and arm.

    python3 tools/spmm_ab.py [--grid 300] [--rounds 10] [--per 5] [--pair] [--out profiles/spmm/spmm_ab.jsonl]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_BYTES_PER_S = 8e12  # MI355X peak


def timed(fn, per, stream):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--pair", action="store_true", help="also time the 16-byte pair variant (AIJHIP_SPMM_PAIR=1)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spmm" / "spmm_ab.jsonl"))
    args = ap.parse_args()
    assert args.rounds * args.per >= 50, "at least 50 timed launches per arm"
    pkg = importlib.import_module("petsc-openacc_amd")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    handles = {}
    handles["templates"], _ = pkg.poisson_device(args.grid)
    handles["csr"], _ = pkg.poisson_device(args.grid)
    for opt in ("row_templates", "row_patterns", "column_codes"):
        handles["csr"].set_option(opt, 0)
    want_path = {"templates": 2, "csr": 1}
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    with out.open("w") as f:
        for name, A in handles.items():
            info = A.info()
            print(f"spmm_ab: {name}: {info}", file=sys.stderr, flush=True)
            n, m = A.n, A.m
            y = torch.empty(m, dtype=torch.float64, device=dev)
            for k in args.ks:
                for layout in ("interleaved", "columns"):
                    plan = A.mat_mult_plan(k, layout)
                    assert plan["path"] == want_path[name], (name, plan)
                    shape = (n, k) if layout == "interleaved" else (k, n)
                    Xs = torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * 2 - 1
                    Ys = torch.empty((m, k) if layout == "interleaved" else (k, m), dtype=torch.float64, device=dev)
                    X, Y = (Xs, Ys) if layout == "interleaved" else (Xs.t(), Ys.t())
                    xcols = [X[:, j].contiguous() for j in range(k)]  # the k MatMults read contiguous vectors

                    def mm8():
                        os.environ["AIJHIP_SPMM_PAIR"] = "0"
                        A.mat_mult(X, Y)

                    def mm16():
                        os.environ["AIJHIP_SPMM_PAIR"] = "1"
                        A.mat_mult(X, Y)

                    def kmults():
                        for xj in xcols:
                            A.mult(xj, y)

                    arms = {"matmat_8B": mm8, "k_mults": kmults}
                    if args.pair and layout == "interleaved":
                        arms["matmat_16B"] = mm16
                    # warm-up of every shape, and the results at the timed size: bit for bit mult's
                    equal = {}
                    for arm, fn in arms.items():
                        for _ in range(3):
                            fn()
                        if arm != "k_mults":
                            Y.fill_(float("nan"))
                            fn()
                            ok = True
                            for j, xj in enumerate(xcols):
                                A.mult(xj, y)
                                ok = ok and bool(torch.equal(Y[:, j].contiguous().view(torch.int64), y.view(torch.int64)))
                            equal[arm] = ok
                    torch.cuda.synchronize()
                    times = {arm: [] for arm in arms}
                    for _ in range(args.rounds):
                        for arm, fn in arms.items():
                            times[arm].extend(timed(fn, args.per, stream))
                    os.environ.pop("AIJHIP_SPMM_PAIR", None)
                    base = statistics.median(times["k_mults"])
                    for arm, t in times.items():
                        med = statistics.median(t)
                        nbytes = plan["bytes"] if arm != "k_mults" else k * info["mult_layout_bytes"]
                        rec = {"grid": args.grid, "plan": name, "path": plan["path"], "layout": layout, "k": k,
                               "arm": arm, "launches": len(t), "us_median": round(med, 2), "us_min": round(min(t), 2),
                               "us_max": round(max(t), 2), "bytes": nbytes,
                               "frac_8TBs": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4),
                               "ratio_to_k_mults": round(med / base, 4)}
                        if arm in equal:
                            rec["bitwise_equal_to_mult"] = equal[arm]
                        line = json.dumps(rec)
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()
                    del Xs, Ys, X, Y, xcols
    for A in handles.values():
        A.destroy()


if __name__ == "__main__":
    main()
