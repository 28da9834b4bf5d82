#!/usr/bin/env python3
"""KSPMatSolve against k KSPSolves on one handle, in one process:
CG + Jacobi on the 7-point Poisson operand assembled on the device, max_it
fixed (rtol = atol = 0, so every iteration runs), k in {2, 4, 8} interleaved
right-hand sides. Once on the CSR plan (row_patterns = 0, which also turns the
row templates off: MatMatMult's path 1) and once on the automatic plan (row
templates, path 2). For each case one mat_solve of the block and the k solves
of its columns on the same handle are warmed up, then timed in turn, round
after round, by the wall clock around the synchronous calls. The single solves
are the handle's own form (fused p.w, and on row templates Z not stored), so
the ratio is what a caller gains or loses by switching calls. One JSON line.

--pc gamg: CG + GAMG instead (a handle with mat_vcycle = max k), solved to
the reference's tolerances (rtol 1e-14, atol 1e-12) rather than for a fixed
count: one mat_solve of the block against the k fused single solves of its
columns; the output goes to profiles/kspmat/ksp_matsolve_gamg_ab.json.

    python3 tools/ksp_matsolve_ab.py [--pc jacobi|gamg] [--grid 300] [--max-it 200] [--rounds 3] [--ks 2 4 8] [--plans csr auto] [--out profiles/kspmat/ksp_matsolve_ab.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_BYTES_PER_S = 8e12  # MI355X peak


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--max-it", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--plans", nargs="+", default=["csr", "auto"], choices=["csr", "auto"])
    ap.add_argument("--pc", default="jacobi", choices=["jacobi", "gamg"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gamg = args.pc == "gamg"
    if args.out is None:
        args.out = str(ROOT / "profiles" / "kspmat" / ("ksp_matsolve_gamg_ab.json" if gamg else "ksp_matsolve_ab.json"))
    solver = dict(rtol=1e-14, atol=1e-12, max_it=10000, pc="gamg", mat_vcycle=max(args.ks)) if gamg else \
        dict(rtol=0.0, atol=0.0, max_it=args.max_it, pc="jacobi")
    pkg = importlib.import_module("petsc-openacc_amd")
    K = importlib.import_module("petsc-openacc_amd.ksp")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    cases = []
    for plan, want_path in (("csr", 1), ("auto", 2)):
        if plan not in args.plans:
            continue
        A, _ = pkg.poisson_device(args.grid)
        if plan == "csr":
            A.set_option("row_patterns", 0)
        m = A.m
        with K.KSPCG(A, **solver) as ksp:
            ksp.set_up()
            info = A.info()
            print(f"ksp_matsolve_ab: {plan}: {info}", file=sys.stderr, flush=True)
            single_bytes = ksp.iteration_bytes()[0]
            for k in args.ks:
                path = A.mat_mult_plan(k, "interleaved")["path"]
                assert path == want_path, (plan, path)
                B = torch.rand((m, k), dtype=torch.float64, device=dev, generator=gen) * 2 - 1
                rhs = torch.empty(m, dtype=torch.float64, device=dev)
                pkg.poisson_vectors_device(args.grid, rhs=rhs)
                B[:, 0] = rhs  # the benchmark's right-hand side beside seeded uniform ones
                X = torch.empty_like(B)
                bcols = [B[:, j].contiguous() for j in range(k)]
                x = torch.empty(m, dtype=torch.float64, device=dev)
                single = []

                def lock_step():
                    ksp.mat_solve(B, X)

                def k_solves():
                    single.clear()
                    for bj in bcols:
                        ksp.solve(bj, x)
                        single.append((ksp.its, ksp.reason))

                arms = {"mat_solve": lock_step, "k_solves": k_solves}
                for fn in arms.values():  # warm-up (the first mat_solve also allocates the work vectors)
                    fn()
                times = {arm: [] for arm in arms}
                for _ in range(args.rounds):
                    for arm, fn in arms.items():
                        times[arm].append(wall(fn))
                lock_step()
                res = ksp.mat_results()
                t_mat = statistics.median(times["mat_solve"])
                t_k = statistics.median(times["k_solves"])
                its = max(r[0] for r in res)
                nbytes, spmm_bytes = ksp.mat_solve_bytes(k)
                # the k solves' bytes: each column's own iteration count
                k_its = sum(i for i, _ in single) / k
                rec = {"grid": args.grid, "pc": args.pc, "plan": plan, "spmm_path": path, "k": k,
                       "max_it": solver["max_it"],
                       "mat_solve_s": round(t_mat, 4), "k_solves_s": round(t_k, 4),
                       "mat_solve_s_all": [round(t, 4) for t in times["mat_solve"]],
                       "k_solves_s_all": [round(t, 4) for t in times["k_solves"]],
                       "ratio_to_k_solves": round(t_mat / t_k, 4),
                       "mat_solve_its_reason": sorted(set((r[0], r[1]) for r in res)),
                       "k_solves_its_reason": sorted(set(single)),
                       "spmm_share_of_bytes": round(spmm_bytes / nbytes, 4),
                       "mat_solve_bytes_per_iter": nbytes, "spmm_bytes_per_iter": spmm_bytes,
                       "k_solves_bytes_per_iter": k * single_bytes, "single_fused": ksp.fused,
                       "mat_solve_frac_8TBs": round(nbytes * its / t_mat / HBM_BYTES_PER_S, 4),
                       "k_solves_frac_8TBs": round(k * single_bytes * k_its / t_k / HBM_BYTES_PER_S, 4),
                       "host_syncs": ksp.host_syncs}
                print(f"ksp_matsolve_ab: {rec}", file=sys.stderr, flush=True)
                cases.append(rec)
                del B, X, bcols, x, rhs
                torch.cuda.empty_cache()
        A.destroy()
    line = json.dumps({"tool": "ksp_matsolve_ab", "device": torch.cuda.get_device_name(0), "cases": cases})
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
