#!/usr/bin/env python3
"""Device BiCGStab (KSPBCGS, AIJHIP_KSP_BCGS) against the same iteration
composed from what a caller has without it (DESIGN §6 "BiCGStab"): A.mult,
KSPCG.pc_apply and torch vector operations, with one host read per dot
product (five per iteration: v.rp, s.t, t.t, r.r, r.rp).

The operand is the tests' convection-diffusion operator at --grid^3: the
7-point Poisson operator assembled on the device with its column row - 1
entries times (1 + c) and its column row + 1 entries times (1 - c), c = 0.3,
once from the automatic layout and once from plain CSR (row templates, row
patterns, column and value codes off). PC Jacobi and GAMG. Per arm: the
iterations and reason of the solve to --rtol, its wall time once warm,
aijhip_ksp_get_iteration_bytes and the fraction of 8 TB/s that gives, and the
wall time of the composition run for the same number of iterations. One JSON
line.

    python3 tools/ksp_bcgs_ab.py [--grid 300] [--rtol 1e-8] [--out profiles/bcgs/ksp_bcgs_ab.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PLAIN_CSR = dict(row_templates=0, row_patterns=0, column_codes=0, value_codes=0)


class DeviceArray:
    """A borrowed device array as torch reads it (__cuda_array_interface__)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def convection_values(A, c, dev):
    """The handle's values with column row - 1 times (1 + c), column row + 1 times (1 - c)."""
    pai, paj, paa = A.device_csr()
    ai = torch.as_tensor(DeviceArray(pai, A.m + 1, "<i4"), device=dev)
    aj = torch.as_tensor(DeviceArray(paj, A.nz, "<i4"), device=dev).long()
    aa = torch.as_tensor(DeviceArray(paa, A.nz, "<f8"), device=dev).clone()
    rows = torch.repeat_interleave(torch.arange(A.m, device=dev), (ai[1:] - ai[:-1]).long())
    aa[aj == rows - 1] *= 1.0 + c
    aa[aj == rows + 1] *= 1.0 - c
    return aa


def composed(A, pc, b, its):
    """`its` BiCGStab iterations from A.mult, pc.pc_apply and torch, every dot
    read on the host. Returns the last preconditioned residual norm."""
    x = torch.zeros_like(b)
    w, r, v, t = (torch.empty_like(b) for _ in range(4))
    pc.pc_apply(b, r)
    rp = r.clone()
    p = torch.zeros_like(b)
    v.zero_()
    rho = torch.dot(r, rp).item()
    rhoold = alpha = omegaold = 1.0
    dp = 0.0
    for _ in range(its):
        beta = (rho / rhoold) * (alpha / omegaold)
        p = r - (omegaold * beta) * v + beta * p
        A.mult(p, w)
        pc.pc_apply(w, v)
        alpha = rho / torch.dot(v, rp).item()
        s = r - alpha * v
        A.mult(s, w)
        pc.pc_apply(w, t)
        omega = torch.dot(s, t).item() / torch.dot(t, t).item()
        x += alpha * p + omega * s
        r = s - omega * t
        dp = torch.dot(r, r).item() ** 0.5
        rhoold, omegaold = rho, omega
        rho = torch.dot(r, rp).item()
    return dp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--c", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bcgs" / "ksp_bcgs_ab.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("petsc-openacc_amd")
    K = importlib.import_module("petsc-openacc_amd.ksp")
    dev = torch.device("cuda:0")
    rec = {"grid": args.grid, "c": args.c, "rtol": args.rtol, "host_reads_per_composed_iteration": 5, "arms": {}}
    rhs = torch.empty(args.grid ** 3, dtype=torch.float64, device=dev)
    pkg.poisson_vectors_device(args.grid, rhs=rhs)
    for layout, options in (("auto", {}), ("csr", PLAIN_CSR)):
        A, _ = pkg.poisson_device(args.grid)
        for k, v in options.items():
            A.set_option(k, v)
        A.update_values_device(convection_values(A, args.c, dev))
        info = A.info()
        for pc in ("jacobi", "gamg"):
            tol = dict(rtol=args.rtol, atol=1e-50, max_it=5000, pc=pc)
            x = torch.zeros_like(rhs)
            with K.KSPBCGS(A, **tol) as ksp, K.KSPCG(A, **tol) as parent:
                t_setup = wall(ksp.set_up)
                ksp.solve(rhs, x)  # warm
                t_solve = wall(lambda: ksp.solve(rhs, x))
                its, reason, rnorm, syncs = ksp.its, ksp.reason, ksp.rnorm, ksp.host_syncs
                nb, nb_spmv, _ = ksp.iteration_bytes()
                res = torch.empty_like(rhs)
                A.mult(x, res)
                true_res = float(torch.linalg.norm(rhs - res) / torch.linalg.norm(rhs))
                parent.set_up()
                composed(A, parent, rhs, min(its, 3))  # warm
                out = {}
                t_comp = wall(lambda: out.setdefault("dp", composed(A, parent, rhs, its)))
            rec["arms"][f"{layout}+{pc}"] = {
                "plan": {k: info.get(k) for k in ("kernel", "row_templates", "row_patterns", "mult_layout_bytes")},
                "its": its, "reason": reason, "rnorm": rnorm, "true_residual_over_b": true_res,
                "host_syncs": syncs, "setup_seconds": round(t_setup, 4), "solve_seconds": round(t_solve, 4),
                "ms_per_iteration": round(t_solve / max(its, 1) * 1e3, 4),
                "iteration_bytes": nb, "spmv_bytes": nb_spmv,
                "GBs": round(nb * its / t_solve / 1e9, 1), "fraction_of_8TBs": round(nb * its / t_solve / 8e12, 4),
                "composed_seconds": round(t_comp, 4), "composed_rnorm": out["dp"],
                "composed_over_device": round(t_comp / t_solve, 3)}
        A.destroy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
