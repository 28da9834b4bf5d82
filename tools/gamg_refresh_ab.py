#!/usr/bin/env python3
"""GAMG reuse-interpolation against the full set-up, in one process (DESIGN §6
"GAMG refresh"): CG + GAMG on the 7-point Poisson operand assembled on the
device, new values supplied through aijhip_mat_update_values_device (no PCIe),
aijhip_ksp_set_up timed by HIP-synchronised wall clocks with the flag off (a
full set-up: today's behaviour, the same code) and on (a refresh), the two
alternated, the median of --rounds each. Three arms:

  scaled    values x 2 and back: the operand stays on row templates;
  variable  S A S, S = diag(u), u uniform in [0.5, 2], two seeds in turn: the
            coefficients are no longer constant, the plan falls to row patterns
            (and the near-null space moves from the constants to S^-1 1, which
            the kept prolongators do not follow);
  drift     the same with u in [0.95, 1.05]: values that drift a little.

Also recorded: the AIJHIP_GAMG_LOG phase lines of one refresh per arm, the
device memory the kept A P patterns hold (hipMemGetInfo around the first
refresh of a handle set up without the flag, which makes and keeps them), and
in every arm the iterations and solve
time of the refreshed hierarchy against the fresh one. One JSON line.

    python3 tools/gamg_refresh_ab.py [--grid 300] [--rounds 5] [--out profiles/gamg_refresh/gamg_refresh_ab.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


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


def with_phase_log(fn):
    """fn() with AIJHIP_GAMG_LOG set; returns the lines it wrote to stderr."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["AIJHIP_GAMG_LOG"] = "1"
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            del os.environ["AIJHIP_GAMG_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return [l for l in tmp.read().decode(errors="replace").splitlines() if l.strip()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gamg_refresh" / "gamg_refresh_ab.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("petsc-openacc_amd")
    K = importlib.import_module("petsc-openacc_amd.ksp")
    dev = torch.device("cuda:0")
    tol = dict(rtol=1e-14, atol=1e-12, max_it=10000, pc="gamg")
    rec = {"grid": args.grid, "rounds": args.rounds, "arms": {}}

    def pair(flag):
        """(A, ksp, seconds of its first set-up)."""
        A, _ = pkg.poisson_device(args.grid)
        ksp = K.KSPCG(A, reuse_interpolation=flag, **tol)
        return A, ksp, wall(ksp.set_up)

    A_off, k_off, t_off0 = pair(False)
    A_on, k_on, t_on0 = pair(True)
    rec["first_setup_seconds"] = {"flag_off": round(t_off0, 4), "flag_on": round(t_on0, 4)}
    rec["levels"] = k_on.pc_levels()[:2]
    m, nz = A_on.m, A_on.nz
    pai, paj, paa = A_on.device_csr()
    ai = torch.as_tensor(DeviceArray(pai, m + 1, "<i4"), device=dev)
    aj = torch.as_tensor(DeviceArray(paj, nz, "<i4"), device=dev).long()
    aa0 = torch.as_tensor(DeviceArray(paa, nz, "<f8"), device=dev).clone()
    # the device memory the kept A P patterns hold: the flag set on the handle
    # that was set up without it, so its first refresh makes the patterns and
    # keeps them (everything else it allocates is freed or replaced in size);
    # a full set-up with the flag off drops them again
    torch.cuda.synchronize()
    free_a = torch.cuda.mem_get_info()[0]
    k_off.reuse_interpolation = True
    A_off.update_values_device(aa0)
    rec["first_refresh_with_symbolic_seconds"] = round(wall(k_off.set_up), 5)
    rec["kept_ap_pattern_bytes"] = int(free_a - torch.cuda.mem_get_info()[0])
    k_off.reuse_interpolation = False
    A_off.update_values_device(aa0)
    k_off.set_up()
    assert k_off.setup_counts()[:2] == (2, 1)
    rows = torch.repeat_interleave(torch.arange(m, device=dev), (ai[1:] - ai[:-1]).long())

    def sas(seed, lo=0.5, hi=2.0):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        u = lo + (hi - lo) * torch.rand(m, dtype=torch.float64, device=dev, generator=g)
        return (u[rows] * aa0) * u[aj]

    rhs = torch.empty(m, dtype=torch.float64, device=dev)
    pkg.poisson_vectors_device(args.grid, rhs=rhs)
    arms = (("scaled", [2.0 * aa0, aa0]), ("variable", [sas(11), sas(12)]),
            ("drift", [sas(21, 0.95, 1.05), sas(22, 0.95, 1.05)]))
    for arm, values in arms:
        t_full, t_ref = [], []
        for r in range(args.rounds + 1):  # round 0 warms both paths up
            v = values[r % 2]
            for A, ksp, out in ((A_off, k_off, t_full), (A_on, k_on, t_ref)):
                A.update_values_device(v)
                t = wall(ksp.set_up)
                if r:
                    out.append(t)
        v = values[(args.rounds + 1) % 2]
        A_on.update_values_device(v)
        lines = with_phase_log(k_on.set_up)
        A_off.update_values_device(v)
        k_off.set_up()
        full, ref, _ = k_on.setup_counts()
        entry = {"full_setup_seconds": [round(t, 5) for t in t_full], "refresh_seconds": [round(t, 5) for t in t_ref],
                 "full_median": round(statistics.median(t_full), 5), "refresh_median": round(statistics.median(t_ref), 5),
                 "refresh_over_full": round(statistics.median(t_ref) / statistics.median(t_full), 4),
                 "plan": {k: A_on.info().get(k) for k in ("row_templates", "row_patterns")},
                 "setup_counts_flag_on": [full, ref], "setup_counts_flag_off": list(k_off.setup_counts()[:2]),
                 "refresh_phase_lines": lines}
        # the fresh hierarchy against the refreshed one, on the same values
        solves, xs = {}, []
        for name, ksp in (("fresh", k_off), ("refreshed", k_on)):
            x = torch.zeros_like(rhs)
            ksp.solve(rhs, x)  # warm
            x.zero_()
            t = wall(lambda: ksp.solve(rhs, x))
            solves[name] = {"its": ksp.its, "reason": ksp.reason, "rnorm": ksp.rnorm, "solve_seconds": round(t, 4)}
            xs.append(x)
        if arm == "scaled":
            # a power of two commutes with every rounding, the prolongator's smoothing included:
            # the fresh hierarchy IS the refreshed one, and the solutions have the same bits
            solves["x_bits_equal"] = bool(torch.equal(xs[0].view(torch.int64), xs[1].view(torch.int64)))
        entry["solve"] = solves
        rec["arms"][arm] = entry
    for h in (k_off, k_on, A_off, A_on):
        h.destroy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
