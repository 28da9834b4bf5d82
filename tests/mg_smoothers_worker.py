"""Worker processes of tests/test_mg_smoothers_gpu.py: CG + GAMG with a level
smoother through the distributed handle (aijhip_kspmpi over the host
transport), ranks as processes sharing cuda:0 — tests/test_gamg_mpi_gpu.py's
runner with the smoother passed on, and at one rank the single-GPU KSPCG
beside it (tests/test_solver_parity_gpu.py's comparison)."""
import importlib
import os
import socket

import numpy as np

TOL = dict(rtol=1e-14, atol=1e-12)  # configs/cg_gamg.info


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, smoother, env, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.update(env)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("petsc-openacc_amd")
        mp_mod = importlib.import_module("petsc-openacc_amd.mpiaij")
        C = importlib.import_module("petsc-openacc_amd.comm")
        K = importlib.import_module("petsc-openacc_amd.ksp")
        dev = torch.device("cuda:0")
        bounds = [mp_mod.slab_bounds(N, world, r) for r in range(world)]
        row_starts = np.array([b[0] * N * N for b in bounds] + [N ** 3], dtype=np.int64)
        z0, z1 = bounds[rank]
        ai, aj, aa = pkg.poisson_csr(N, N, N, z0, z1)

        def make_local(a_i, a_j, a_a, ncols):
            return pkg.SeqAIJHIP(a_i, a_j, a_a, ncols=ncols)

        comm = C.Comm.host(device=0, timeout_s=120)
        op = mp_mod.MPIAIJ(ai, aj, aa, row_starts, make_local, pkg.split_rows, dev, comm=comm)
        rhs, _ = pkg.poisson_vectors(N, N, N, z0, z1)
        b = torch.from_numpy(rhs).to(dev)
        x = torch.full_like(b, float("nan"))
        with C.KSPCGMPINative(op.p2p_native() if world > 1 else op.native, max_it=1000, pc="gamg",
                              smoother=smoother, **TOL) as k:
            k.solve(b, x)
            torch.cuda.synchronize()
            out = dict(x=x.cpu().numpy(), its=k.its, reason=k.reason, hist=np.array(k.hist), rows=k.pc_levels()[0])
        if world == 1:  # the single-GPU handle on the same operand
            xs = torch.full_like(b, float("nan"))
            with pkg.SeqAIJHIP(ai, aj, aa) as A, K.KSPCG(A, max_it=1000, pc="gamg", smoother=smoother, **TOL) as ksp:
                ksp.solve(b, xs)
                torch.cuda.synchronize()
                out["single"] = dict(x=xs.cpu().numpy(), its=ksp.its, reason=ksp.reason,
                                     hist=np.array(ksp.history()), smoother=ksp.mg_smoother(0))
        q.put((rank, out))
    except Exception as e:  # noqa: BLE001
        q.put((rank, {"error": repr(e)}))
    finally:
        dist.destroy_process_group()


def run(world, N, smoother, env=None):
    """{rank: result} of `world` (at most 2) ranks solving the N^3 problem in z slabs."""
    import torch.multiprocessing as mp
    assert world <= 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, N, smoother, env or {}, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=300)
            got[r] = out
    finally:
        for p in procs:
            p.join(timeout=120)
    for r in range(world):
        assert "error" not in got[r], got[r]["error"]
    for p in procs:
        assert p.exitcode == 0
    return got
