"""The distributed CG handle on one rank against the single-GPU KSPCG.

On one rank the row-partitioned solver (aijhip_kspmpi over the host
transport, Comm.host) has no ghost rows and no all-reduce: it runs the same
CG driver, the same kernels and the same fixed-order sums as the single-GPU
KSP, so x agrees bit for bit and its / reason / residual history are
identical — for every PC the distributed wrapper accepts, every norm, and a
solve cut short inside the first poll batch (max_it = 3: DIVERGED_ITS, the
deferred X += a P applied by the final pass) as well as a converged one.

One worker process per case group (operand size), every case of the group in
it; pc = bjacobi_gamg at one rank is PCGAMG on the whole operator, so its
single-GPU counterpart is pc = gamg."""
import importlib
import itertools
import os
import socket

import numpy as np
import pytest

NORMS = ("preconditioned", "unpreconditioned", "natural")
MAX_ITS = (3, 2000)
# group -> (N, the cases (pc, norm, max_it) solved on the N^3 Poisson operand)
GROUPS = {
    "jacobi12": (12, list(itertools.product(("none", "jacobi"), NORMS, MAX_ITS))),
    "gamg20": (20, list(itertools.product(("gamg", "bjacobi_gamg"), NORMS, MAX_ITS))),
    # the finest level's coarsening is built on the device
    "gamg40": (40, [("gamg", "preconditioned", 2000)]),
}
CASES = [(g, *c) for g, (_, cs) in GROUPS.items() for c in cs]
DIVERGED_ITS = -3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(port, N, cases, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        pkg = importlib.import_module("petsc-openacc_amd")
        mp_mod = importlib.import_module("petsc-openacc_amd.mpiaij")
        C = importlib.import_module("petsc-openacc_amd.comm")
        K = importlib.import_module("petsc-openacc_amd.ksp")
        dev = torch.device("cuda:0")
        comm = C.Comm.host(device=0, timeout_s=60)
        ai, aj, aa = pkg.poisson_csr(N)
        row_starts = np.array([0, N ** 3], np.int64)

        def make_local(a_i, a_j, a_a, ncols):
            return pkg.SeqAIJHIP(a_i, a_j, a_a, ncols=ncols)

        op = mp_mod.MPIAIJ(ai, aj, aa, row_starts, make_local, pkg.split_rows, dev, comm=comm)
        A = pkg.SeqAIJHIP(ai, aj, aa)
        rhs, _ = pkg.poisson_vectors(N)
        b = torch.from_numpy(rhs).to(dev)
        out = {}
        for pc, norm, max_it in cases:
            xn = torch.full_like(b, float("nan"))
            with C.KSPCGMPINative(op.native, rtol=1e-12, max_it=max_it, norm=norm, pc=pc) as kn:
                kn.solve(b, xn)
                nat = dict(its=kn.its, reason=kn.reason, hist=np.array(kn.hist))
            xs = torch.full_like(b, float("nan"))
            with K.KSPCG(A, rtol=1e-12, max_it=max_it, norm=norm,
                         pc="gamg" if pc == "bjacobi_gamg" else pc) as ksp:
                ksp.solve(b, xs)
                single = dict(its=ksp.its, reason=ksp.reason, hist=np.array(ksp.history()))
            torch.cuda.synchronize()
            out[(pc, norm, max_it)] = dict(nat=nat, single=single, x_same=bool(torch.equal(xn, xs)),
                                           x_finite=bool(torch.isfinite(xs).all()))
        q.put(out)
    except Exception as e:  # noqa: BLE001
        q.put({"error": repr(e)})
    finally:
        dist.destroy_process_group()


_results = {}


def _group(name):
    """Every case of a group, solved once in one worker process."""
    if name not in _results:
        import torch.multiprocessing as mp
        N, cases = GROUPS[name]
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        p = ctx.Process(target=_worker, args=(_free_port(), N, cases, q))
        p.start()
        try:
            r = q.get(timeout=300)
        finally:
            p.join(timeout=120)
        if "error" not in r and p.exitcode != 0:
            r = {"error": f"worker exit code {p.exitcode}"}
        _results[name] = r
    return _results[name]


@pytest.mark.gpu
@pytest.mark.parametrize("group,pc,norm,max_it", CASES)
def test_gpu_distributed_cg_on_one_host_rank_matches_single_gpu_bitwise(group, pc, norm, max_it):
    r = _group(group)
    assert "error" not in r, r.get("error")
    c = r[(pc, norm, max_it)]
    nat, single = c["nat"], c["single"]
    print(f"\n{group} {pc} {norm} max_it={max_it}: its {nat['its']} / {single['its']}, "
          f"reason {nat['reason']} / {single['reason']}")
    assert nat["its"] == single["its"] and nat["reason"] == single["reason"]
    assert nat["hist"].shape == single["hist"].shape
    assert np.array_equal(nat["hist"].view(np.uint64), single["hist"].view(np.uint64))
    assert c["x_finite"] and c["x_same"]
    if max_it == 3:  # stopped inside the first poll batch
        assert single["reason"] == DIVERGED_ITS and single["its"] == 3
    else:
        assert single["reason"] > 0 and single["its"] > 3
