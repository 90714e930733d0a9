"""N>1 path on CPU: the single per-outer-iteration exchange of sharded runs over `gloo`
(world_size 2), and -- on the GPU box -- two ranks driving the real LM loop with that exchange
(frozen-rank protocol: a rank that converged keeps taking part until all have)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lsq_amd as lsq


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _worker_exchange(rank, world, port, q):
    _init(rank, world, port)
    buf = torch.zeros(world + lsq.sharding.NSLOT, dtype=torch.float64)
    out = []
    # rank r contributes ssr = r+1, gnorm = 10*(r+1); only rank 0 has converged in round 0
    out.append(lsq.sharding.exchange(dist, rank, world, rank + 1.0, 10.0 * (rank + 1), rank == 0, buf))
    out.append(lsq.sharding.exchange(dist, rank, world, 0.5, 0.25 if rank else 7.0, True, buf))
    cb = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    import ctypes as C
    vals = (C.c_double * 3)(2.0 * (rank + 1), 3.0 - rank, 1.0)
    assert cb(vals, 3, None) == 0
    out.append((vals[0], vals[1], vals[2]))
    # active ranks (converged = 0): the first call is synchronous, later ones return the PREVIOUS exchange
    # while their own all-reduce stays in flight; a converged call drains it and is synchronous again
    cb2 = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    seq = []
    for it, conv in enumerate([0.0, 0.0, 0.0, 1.0]):
        vals = (C.c_double * 3)(10.0 * it + rank, float(it + rank), conv)
        assert cb2(vals, 3, None) == 0
        seq.append((vals[0], vals[1], vals[2]))
    out.append(seq)
    # error protocol: rank 1 leaves with an error (converged = -1) at its 3rd call; rank 0 (active, one exchange in
    # flight) learns of it at its 4th call BEFORE issuing another collective: both ranks issue exactly 3 all-reduces
    cb3 = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    rcs = []
    for it in range(5):
        leaving = rank == 1 and it == 2
        vals = (C.c_double * 3)(1.0, 1.0, -1.0 if leaving else 0.0)
        rcs.append(cb3(vals, 3, None))
        if leaving or rcs[-1] == 2:
            break
    out.append(rcs)
    lsq.sharding.drain_all()
    dist.barrier()
    q.put((rank, out))
    dist.destroy_process_group()


def test_exchange_gloo_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_exchange, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        assert res[r][0] == (3.0, 20.0, False)          # sum, max, not all converged
        assert res[r][1] == (1.0, 7.0, True)
        assert res[r][2] == (6.0, 3.0, 1.0)
        # sums over ranks {0,1}: iteration it contributes 20*it + 1, max gnorm it + 1
        assert res[r][3] == [(1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (21.0, 2.0, 0.0), (61.0, 4.0, 1.0)]
    assert res[1][4] == [0, 0, 0]            # the leaving rank: its last call succeeds
    assert res[0][4] == [0, 0, 0, 2]         # its peer: told at the next call, no further collective


def _scripts(rank):
    """Made-up per-iteration inputs {ssr, |g|, state} of rank `rank` (state: 0 active, 1 converged, -1 leaving)."""
    a = [(10.0 * it + rank, float(it + rank), c) for it, c in enumerate([0.0, 0.0, 0.0, 1.0])]
    # the ranks converge at different iterations: rank 0 freezes at call 2, rank 1 at call 5
    b = [(1.0 / (it + 1) + rank, 3.0 - 0.5 * it + rank, 1.0 if it >= (2 if rank == 0 else 5) else 0.0) for it in range(7)]
    # rank 1 leaves with an error at its 3rd call
    c = [(1.0, 1.0 + rank, -1.0 if (rank == 1 and it == 2) else 0.0) for it in range(5)]
    # rank 0 leaves at the very first call
    d = [(2.0, 0.5, -1.0 if (rank == 0 and it == 0) else 0.0) for it in range(3)]
    return [a, b, c, d]


def _drive(cb, script):
    import ctypes as C
    seq = []
    for ssr, gn, state in script:
        vals = (C.c_double * 3)(ssr, gn, state)
        rc = cb(vals, 3, None)
        seq.append((rc, vals[0], vals[1], vals[2]))
        if state < -0.5 or rc != 0:
            break
    return seq


def _worker_c_vs_python(rank, world, port, q):
    _init(rank, world, port)
    out = []
    for script in _scripts(rank):
        py = _drive(lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu"), script)
        lsq.sharding.drain_all()
        dist.barrier()
        x = lsq.sharding.TorchTransportExchange(dist, rank, world)
        cc = _drive(x, script)
        x.drain()
        st = x.stats()
        x.close()
        dist.barrier()
        out.append((py, cc, st))
    q.put((rank, out))
    dist.destroy_process_group()


def test_c_exchange_equals_python_hook_gloo_world2():
    """lsq_options.allreduce served in C (liblsqrccl.so: lsq_rccl_xchg_*, here over a gloo transport through
    lsq_rccl_xchg_create_custom) against its Python twin (sharding.make_allreduce_callback) on the same made-up scalars,
    world 2: the same return code and the same three values at EVERY call -- first call synchronous, active ranks get the
    previous exchange, frozen ranks this one, a leaving rank stops everybody with the same number of collectives."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_c_vs_python, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        for k, (py, cc, st) in enumerate(res[r]):
            assert py == cc, (r, k, py, cc)
            assert st["collectives"] <= len(cc)
    # script a, both ranks: sums over ranks {0,1}: iteration it contributes 20*it + 1, max gnorm it + 1
    assert [v[1:] for v in res[0][0][1]] == [(1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (21.0, 2.0, 0.0), (61.0, 4.0, 1.0)]
    # script c: the leaving rank's last call succeeds, its peer is told at its next call; both issued 3 collectives
    assert [v[0] for v in res[1][2][1]] == [0, 0, 0] and [v[0] for v in res[0][2][1]] == [0, 0, 0, 2]
    assert res[0][2][2]["collectives"] == res[1][2][2]["collectives"] == 3 and res[0][2][2]["aborted"]
    # script d: rank 0 leaves at once (rc 0), rank 1's synchronous first call sees it: rc 2, one collective each
    assert [v[0] for v in res[0][3][1]] == [0] and [v[0] for v in res[1][3][1]] == [2]
    assert res[0][3][2]["collectives"] == res[1][3][2]["collectives"] == 1


def _scripts_world8(rank, world):
    """Round 6: made-up inputs for EIGHT ranks.  a: staggered convergence -- rank r freezes at call 2 + r, so
    for most of the run some ranks are active (previous-result semantics, exchange in flight) while others are frozen
    (synchronous calls), and the run ends at the call in which the slowest rank reports convergence.  b: one rank (5) leaves
    with an error at its 4th call while ranks 0..2 are already frozen and the others active: every rank must stop with the
    same number of collectives.  c: the LAST rank leaves at the very first call."""
    a = [(1.0 / (it + 1) + rank, 10.0 - 0.5 * it + rank, 1.0 if it >= 2 + rank else 0.0) for it in range(world + 4)]
    b = [(2.0 + rank, 1.0 + it, -1.0 if (rank == 5 and it == 3) else (1.0 if it >= 1 + rank and rank < 3 else 0.0)) for it in range(8)]
    c = [(1.0, 0.5, -1.0 if (rank == world - 1 and it == 0) else 0.0) for it in range(3)]
    return [a, b, c]


def _worker_c_vs_python_world8(rank, world, port, q):
    _init(rank, world, port)
    out = []
    for script in _scripts_world8(rank, world):
        py = _drive(lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu"), script)
        lsq.sharding.drain_all()
        dist.barrier()
        x = lsq.sharding.TorchTransportExchange(dist, rank, world)
        cc = _drive(x, script)
        x.drain()
        st = x.stats()
        x.close()
        dist.barrier()
        out.append((py, cc, st))
    q.put((rank, out))
    dist.destroy_process_group()


def test_c_exchange_gloo_world8_staggered_and_abort():
    """C5 readiness without an 8-GPU node: the exchange protocol served in C (liblsqrccl.so through
    lsq_rccl_xchg_create_custom, gloo transport) at the world size of BASELINE's C5 -- eight ranks, staggered convergence, one
    aborting rank -- against its Python twin call by call, with equal collective counts on every rank."""
    world, port = 8, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_c_vs_python_world8, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        for k, (py, cc, st) in enumerate(res[r]):
            assert py == cc, (r, k, py, cc)
    # script a: everybody leaves at the call in which the slowest rank (7: call index 9) reports convergence, with "all
    # converged" and the global sum / max of THAT call; nobody aborted; the collective counts agree
    na = 2 + (world - 1) + 1
    for r in range(world):
        cc, st = res[r][0][1], res[r][0][2]
        assert len(cc) >= na and all(v[0] == 0 for v in cc[:na])
        assert cc[na - 1][3] == 1.0 and all(v[3] == 0.0 for v in cc[:na - 1])
        assert cc[na - 1][1] == pytest.approx(sum(1.0 / na + k for k in range(world)), rel=1e-15)
        assert not st["aborted"]
    assert len({res[r][0][2]["collectives"] for r in range(world)}) == 1
    # script b: rank 5 leaves at its 4th call (rc 0 for itself); every other rank is told (rc 2) at its 4th or 5th call, and ALL
    # ranks have issued the same number of collectives
    assert [v[0] for v in res[5][1][1]] == [0, 0, 0, 0]
    for r in range(world):
        if r != 5:
            rcs = [v[0] for v in res[r][1][1]]
            assert rcs[-1] == 2 and all(v == 0 for v in rcs[:-1]) and len(rcs) in (4, 5), (r, rcs)
        assert res[r][1][2]["aborted"]
    assert len({res[r][1][2]["collectives"] for r in range(world)}) == 1
    # script c: the last rank leaves at once; everybody else's synchronous first call sees it; one collective each
    for r in range(world):
        rcs = [v[0] for v in res[r][2][1]]
        assert rcs == ([0] if r == world - 1 else [2]), (r, rcs)
        assert res[r][2][2]["collectives"] == 1


def test_c_exchange_symbols_and_one_rank_protocol():
    """include/lsqrccl.h's exchange entry points are exported, and the protocol at world 1 over the built-in transport double
    (no process group): first call and frozen calls synchronous, active calls return the previous exchange."""
    import ctypes as C
    L = lsq.sharding.rccl_shim()
    for name in ("lsq_rccl_xchg_create", "lsq_rccl_xchg_create_custom", "lsq_rccl_xchg_destroy", "lsq_rccl_xchg_callback",
                 "lsq_rccl_xchg_drain", "lsq_rccl_xchg_reset", "lsq_rccl_xchg_stats"):
        assert hasattr(L, name), name
    x = lsq.sharding.TorchTransportExchange(None, 0, 1)
    seq = _drive(x, [(2.5, 0.3, 0.0), (1.5, 0.2, 0.0), (1.25, 0.1, 0.0), (1.0, 0.05, 1.0)])
    assert seq == [(0, 2.5, 0.3, 0.0), (0, 2.5, 0.3, 0.0), (0, 1.5, 0.2, 0.0), (0, 1.0, 0.05, 1.0)]
    assert x.stats() == {"collectives": 4, "synchronous": 2, "aborted": False}
    # the protocol state is per RUN.  Without a reset an active rank's first call of the next run returns the previous
    # run's final result; lsq_rccl_xchg_reset (api._run_native calls it before every run) makes that call synchronous again
    assert _drive(x, [(3.0, 0.7, 0.0)]) == [(0, 1.0, 0.05, 1.0)]
    x.reset()
    assert _drive(x, [(3.0, 0.7, 0.0), (2.0, 0.6, 0.0)]) == [(0, 3.0, 0.7, 0.0), (0, 3.0, 0.7, 0.0)]
    x.close()


def _worker_lm(rank, world, port, q):
    _init(rank, world, port)
    ctx = lsq.Context(0)
    # two different problems; the second needs more iterations
    m, n = (4000, 40) if rank == 0 else (6000, 60)
    pr = lsq.synthetic.TanhProblem(m, n, sparse=True, per_col=100, seed=11 + rank, ctx=ctx)
    pr.reset()
    cb = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    r = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60, allreduce=cb)
    pr.reset()
    r1 = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60)  # same problem, alone
    q.put((rank, r.iterations, r.converged, r.ssr, r1.iterations, r1.ssr, float(np.max(np.abs(r.minimizer - r1.minimizer)))))
    pr.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_lm_with_exchange():
    """Both ranks leave the loop in the same outer iteration (the slower problem's count), each
    rank's own solution is unchanged by the exchange, and the reported ssr is the global sum."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_lm, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world):
        rec = q.get(timeout=300)
        res[rec[0]] = rec[1:]
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    (it0, c0, ssr0, alone0, s0, d0), (it1, c1, ssr1, alone1, s1, d1) = res[0], res[1]
    assert c0 and c1
    assert it0 == it1 == max(alone0, alone1) + 1 or it0 == it1 == max(alone0, alone1)
    assert d0 == 0.0 and d1 == 0.0                      # local trajectories untouched
    assert ssr0 == pytest.approx(s0 + s1, rel=1e-12) and ssr1 == pytest.approx(ssr0, rel=1e-15)


def _worker_shared_device(rank, world, port, q):
    """Rank 0: a sparse LM+LSMR problem (sliced layouts, look-ahead, speculative tail); rank 1: a C2-sized dense LM+Cholesky
    problem (4096 x 512: the one-launch Cholesky and the pipelined triangular solves, which assume co-resident workgroups).
    Both processes drive the ONE device of the box at the same time and meet in the per-iteration exchange."""
    _init(rank, world, port)
    ctx = lsq.Context(0)
    if rank == 0:
        pr = lsq.synthetic.TanhProblem(400_000, 4000, sparse=True, per_col=400, seed=21, ctx=ctx)
        sol = lsq._lib.LSMR
    else:
        pr = lsq.synthetic.TanhProblem(4096, 512, sparse=False, seed=22, ctx=ctx)
        sol = lsq._lib.CHOLESKY
    cb = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    runs = []
    for rep in range(3):                      # (several runs: the neighbour's kernels land differently every time)
        pr.reset()
        r = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, sol, iterations=12, allreduce=cb, x_tol=0, f_tol=0, g_tol=0)
        runs.append((r.iterations, r.ssr, r.minimizer))
    dist.barrier()                            # the neighbour is done: the device is this process's own
    pr.reset()
    r1 = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, sol, iterations=12, x_tol=0, f_tol=0, g_tol=0)
    q.put((rank, [(it, ssr, float(np.max(np.abs(x - r1.minimizer)) / max(1.0, np.max(np.abs(r1.minimizer))))) for it, ssr, x in runs],
           r1.iterations, r1.ssr, ctx.fallback_stats()))
    pr.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_share_one_device_lsmr_beside_dense_cholesky():
    """C5 readiness without an 8-GPU node: two ranks of the independent-problem LM loop on the ONE device
    of the box -- a sparse LM+LSMR run beside a C2-sized LM+Cholesky run, exchanging once per outer iteration.  The other
    rank's kernels are exactly the neighbour that breaks the co-residency assumptions of the dense fast paths (DESIGN 4.6
    rows 5, 7): whatever they do -- run clean, or give up on a bounded wait and fall back -- every run must reproduce the
    rank's own undisturbed run (LSMR: same kernels, to round-off of nothing: equal bits; Cholesky: to 1e-9, the fall-back
    factors in another order), with the global ssr in every rank's result."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_shared_device, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world):
        rec = q.get(timeout=600)
        res[rec[0]] = rec[1:]
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    for rep in range(3):
        (it0, ssr0, d0), (it1, ssr1, d1) = res[0][0][rep], res[1][0][rep]
        assert it0 == it1 == 12
        assert ssr0 == pytest.approx(res[0][2] + res[1][2], rel=1e-9) and ssr1 == pytest.approx(ssr0, rel=1e-15)
        assert d0 == 0.0, ("sparse LM+LSMR beside a neighbour", rep, d0)
        assert d1 <= 1e-9, ("dense LM+Cholesky beside a neighbour", rep, d1, res[1][3])


def _worker_lm_failing(rank, world, port, q, fail_at_f_call, iterations):
    """Rank 1's f! fails at its `fail_at_f_call`-th call (call 1 = f(x0), call k+1 = the trial point of iteration k)."""
    import ctypes as C
    _init(rank, world, port)
    os.environ["LSQ_EXCHANGE_TIMEOUT_S"] = "20"
    ctx = lsq.Context(0)
    pr = lsq.synthetic.TanhProblem(4000, 40, sparse=True, per_col=100, seed=21 + rank, ctx=ctx)
    pr.reset()
    L = lsq.lib()
    model_f = L.lsq_model_f()
    calls = [0]

    def f(d_out, d_x, user):
        calls[0] += 1
        if rank == 1 and calls[0] == fail_at_f_call:
            return 1
        return model_f(d_out, d_x, user)

    class _H:
        pass

    Jd = _H()
    Jd.h = pr.J
    cb = lsq.sharding.make_allreduce_callback(dist, rank, world, "cpu")
    st, res, _ = lsq.api._run_native(ctx, lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, Jd, pr.x, pr.fcur,
                                     lsq._lib.F_CALLBACK(f), L.lsq_model_g(), pr.model, 0.0, 0.0, 0.0, iterations, None,
                                     None, None, False, pr.n, allreduce=cb)
    lsq.sharding.drain_all()
    q.put((rank, st, res.iterations, calls[0]))
    pr.close()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("when", ["last_iteration", "mid_run"])
def test_rank_failing_after_its_exchange_does_not_hang(when):
    """a rank whose callback fails in its LAST allowed iteration, after that iteration's exchange, must not issue
    a farewell exchange -- its peers are leaving their loops and would never match it (it used to wait forever).  Mid-run
    the farewell IS matched and the peer leaves with LSQ_ERCCL."""
    from lsq_amd import api as _api  # noqa: F401  (lsq.api)
    iterations = 6
    fail_at = 1 + iterations if when == "last_iteration" else 3
    world, port = 2, _free_port()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    ps = [mpc.Process(target=_worker_lm_failing, args=(r, world, port, q, fail_at, iterations)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world):
        rec = q.get(timeout=180)
        res[rec[0]] = rec[1:]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert res[1][0] == lsq._lib.ECALLBACK and res[1][2] == fail_at
    if when == "last_iteration":
        assert res[0][0] == lsq._lib.OK and res[0][1] == iterations      # the peer finished all its iterations
    else:
        assert res[0][0] == lsq._lib.ERCCL                                # the peer was told and left


def _worker_lm_rccl(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    ctx = lsq.Context(0)
    pr = lsq.synthetic.TanhProblem(6000, 60, sparse=True, per_col=100, seed=12, ctx=ctx)
    pr.reset()
    cb = lsq.sharding.make_allreduce_callback(dist, rank, world, "cuda")     # default group = the nccl (RCCL) group
    r = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60, allreduce=cb)
    lsq.sharding.drain_all()
    pr.reset()
    r1 = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60)
    q.put((dist.get_backend(), dist.get_world_size(), r.iterations, r.converged, r.ssr, r1.iterations, r1.ssr,
           float(np.max(np.abs(r.minimizer - r1.minimizer)))))
    pr.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_lm_with_rccl_exchange_world1():
    """The exchange callback over the `nccl` (= RCCL) backend on real hardware: a one-rank group (a GPU box has one
    device), the same code path bench.py's sharded runs take by default.  The run must equal the unsharded run."""
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_lm_rccl, args=(0, 1, port, q))
    p.start()
    backend, ws, it, conv, ssr, it1, ssr1, d = q.get(timeout=600)
    p.join(120)
    assert p.exitcode == 0
    assert backend == "nccl" and ws == 1
    assert conv and it in (it1, it1 + 1)      # the frozen-rank protocol may add the iteration that sees "all converged"
    assert d == 0.0 and ssr == pytest.approx(ssr1, rel=1e-15)


def _worker_lm_c_exchange(rank, world, port, q, backend):
    """The real LM loop with the exchange served in C: backend "gloo" = the C protocol over a gloo transport (two ranks on the
    one device of the box), "rccl" = lsq_rccl_xchg_create over an RCCL communicator (rank r on device r)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = rank if backend == "rccl" and torch.cuda.device_count() >= world else 0
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = lsq.Context(dev)
    m, n = (4000, 40) if rank == 0 else (6000, 60)
    pr = lsq.synthetic.TanhProblem(m, n, sparse=True, per_col=100, seed=11 + rank, ctx=ctx)
    x = (lsq.sharding.RcclScalarExchange(rank, world, dist) if backend == "rccl" else
         lsq.sharding.TorchTransportExchange(dist, rank, world))
    pr.reset()
    r = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60, allreduce=x)
    x.drain()
    st = x.stats()
    dist.barrier()
    pr.reset()
    r1 = pr.optimize(lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR, iterations=60)
    q.put((rank, r.iterations, r.converged, r.ssr, r1.iterations, r1.ssr, float(np.max(np.abs(r.minimizer - r1.minimizer))), st))
    x.close()
    pr.close()
    dist.destroy_process_group()


def _run_c_exchange(world, backend):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_lm_c_exchange, args=(r, world, port, q, backend)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world):
        rec = q.get(timeout=600)
        res[rec[0]] = rec[1:]
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    return res


@pytest.mark.gpu
def test_lm_with_c_rccl_exchange_world1():
    """lsq_rccl_xchg_* on hardware: a one-rank RCCL communicator (what a one-GPU box offers), ncclAllReduce of 4 doubles per
    outer iteration on the exchange's side stream.  The run equals the unsharded run; every iteration issued one collective."""
    res = _run_c_exchange(1, "rccl")
    it, conv, ssr, it1, ssr1, d, st = res[0]
    assert conv and it in (it1, it1 + 1) and d == 0.0 and ssr == pytest.approx(ssr1, rel=1e-15)
    # one collective per outer iteration + the frozen rank's call that sees "all converged" and leaves
    assert st["collectives"] in (it, it + 1) and not st["aborted"]


@pytest.mark.gpu
def test_two_ranks_lm_with_c_exchange_over_gloo():
    """Two ranks of the real LM loop on the one device, the exchange served by the C protocol (gloo transport): both leave in
    the same outer iteration, local trajectories untouched, global ssr in both results -- as with the Python hook."""
    res = _run_c_exchange(2, "gloo")
    (it0, c0, ssr0, alone0, s0, d0, st0), (it1, c1, ssr1, alone1, s1, d1, st1) = res[0], res[1]
    assert c0 and c1 and it0 == it1 and it0 in (max(alone0, alone1), max(alone0, alone1) + 1)
    assert d0 == 0.0 and d1 == 0.0
    assert ssr0 == pytest.approx(s0 + s1, rel=1e-12) and ssr1 == pytest.approx(ssr0, rel=1e-15)
    assert st0["collectives"] == st1["collectives"] and st0["collectives"] in (it0, it0 + 1)


def _worker_c5_shared(rank, world, port, q):
    """One rank of an 8-rank C5 run squeezed onto the ONE device of the box: a reduced C4 problem (125 000 x 10 000, nnz 1.25e6:
    both sliced layouts, the three-launch LSMR iteration, the speculative tail -- the kernels of the headline), seed 20260928 +
    rank as in bench.py, the exchange served in C over a gloo transport."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = lsq.Context(0)
    pr = lsq.synthetic.TanhProblem(125_000, 10_000, sparse=True, per_col=125, seed=lsq.synthetic.BASE_SEED + rank, ctx=ctx)
    x = lsq.sharding.TorchTransportExchange(dist, rank, world)
    LM, LSMR = lsq._lib.LEVENBERG_MARQUARDT, lsq._lib.LSMR
    dist.barrier()
    pr.reset()
    r = pr.optimize(LM, LSMR, iterations=40, allreduce=x, trace=True)      # default tolerances: the ranks converge on their own
    x.drain()
    st = x.stats()
    dist.barrier()                                                          # the neighbours are done
    pr.reset()
    r1 = pr.optimize(LM, LSMR, iterations=40, trace=True)                   # the same problem, alone on the device
    k = r1.iterations
    same = (np.array_equal(np.array(r.trace["x"])[:k], np.array(r1.trace["x"])[:k]) and
            np.array_equal(np.asarray(r.trace["ssr"])[:k], np.asarray(r1.trace["ssr"])[:k]) and
            np.array_equal(np.asarray(r.trace["inner"])[:k], np.asarray(r1.trace["inner"])[:k]) and
            np.array_equal(np.asarray(r.trace["accept"])[:k], np.asarray(r1.trace["accept"])[:k]))
    q.put((rank, r.iterations, bool(r.converged), float(r.ssr), r1.iterations, bool(r1.converged), float(r1.ssr), bool(same),
           float(np.max(np.abs(r.minimizer - r1.minimizer))), st, ctx.fallback_stats()))
    x.close()
    pr.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_eight_ranks_share_one_device_c5_protocol():
    """C5 readiness without an 8-GPU node: EIGHT processes drive the one device at once, each with its own
    reduced C4 problem and the C exchange over gloo -- eight launch threads contending for the host and the queue, which world 2
    cannot show.  Every rank's trajectory (iterates, ssr, inner counts, accept pattern) is bit-identical to the same problem run
    alone, all ranks leave in the same outer iteration with the global ssr, and all issued the same number of collectives."""
    world, port = 8, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_c5_shared, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world):
        rec = q.get(timeout=900)
        res[rec[0]] = rec[1:]
    for p in ps:
        p.join(180)
        assert p.exitcode == 0
    its = {res[r][0] for r in range(world)}
    alone = [res[r][3] for r in range(world)]
    assert len(its) == 1 and its.pop() in (max(alone), max(alone) + 1)
    total = sum(res[r][5] for r in range(world))
    for r in range(world):
        it, conv, ssr, it1, conv1, ssr1, same, dx, st, fb = res[r]
        assert conv and conv1, r
        assert same and dx == 0.0, ("rank %d: trajectory beside 7 neighbours differs from the run alone" % r, dx)
        assert ssr == pytest.approx(total, rel=1e-12)
        assert not st["aborted"]
    assert len({res[r][8]["collectives"] for r in range(world)}) == 1


@pytest.mark.gpu
def test_two_ranks_lm_with_c_rccl_exchange_world2():
    """C5 over RCCL with N = 2 ranks, one per GPU (runs by itself wherever the box has two devices; skipped on a one-GPU
    lease -- RCCL refuses two ranks on one device)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL: one rank per device)")
    res = _run_c_exchange(2, "rccl")
    (it0, c0, ssr0, alone0, s0, d0, st0), (it1, c1, ssr1, alone1, s1, d1, st1) = res[0], res[1]
    assert c0 and c1 and it0 == it1 and d0 == 0.0 and d1 == 0.0
    assert ssr0 == pytest.approx(s0 + s1, rel=1e-12) and ssr1 == pytest.approx(ssr0, rel=1e-15)
    assert st0["collectives"] == st1["collectives"] and st0["collectives"] in (it0, it0 + 1)


def _bench_line(args, env=None, timeout=900):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=e, timeout=timeout,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines                         # exactly ONE line on stdout
    return json.loads(lines[0])


def test_bench_gpus2_spawns_two_ranks():
    """`python bench.py --gpus 2` with no torchrun environment must itself start 2 ranks (round-1 bug: --gpus was
    parsed and ignored).  --dry-run = the launch path only (no CPU implementation of the hot path exists)."""
    j = _bench_line(["--gpus", "2", "--steps", "6", "--dry-run", "--m", "4000", "--n", "40"])
    assert j["n_gpus"] == 2 and j["config"]["process_group_ranks"] == 2 and j["config"]["problems"] == 2
    assert j["dry_run"] is True and j["value"] is None


def test_bench_rejects_mismatched_world():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run"], env=e,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode != 0 and b"WORLD_SIZE=1" in out.stderr


@pytest.mark.gpu
def test_bench_forced_exchange_runs_on_rccl():
    """bench.py's sharded protocol with its default exchange backend on hardware (one rank: LSQ_BENCH_FORCE_EXCHANGE)."""
    j = _bench_line(["--steps", "8", "--warmup", "8", "--repeats", "3", "--m", "20000", "--n", "200", "--per-col", "100",
                     "--no-cpu"], env={"LSQ_BENCH_FORCE_EXCHANGE": "1"})
    assert j["n_gpus"] == 1 and j["config"]["exchange_backend"] == "rccl-c" and j["config"]["rccl_ranks"] == 1
    assert j["config"]["exchange"]["collectives"] > 0
    assert j["value"] > 0 and j["repeats"] == 3 and j["region_ms"]["min"] <= j["region_ms"]["median"] <= j["region_ms"]["max"]


@pytest.mark.gpu
def test_bench_plain_run_times_k_steps_and_dumps_outputs(tmp_path):
    """A plain `bench.py` run: ONE timed region of exactly --steps steps, the headline only (the companion legs are --full's),
    and --dump-outputs writes what the last timed solve returned."""
    import numpy as np
    m, n = 20000, 200
    j = _bench_line(["--steps", "10", "--warmup", "2", "--m", str(m), "--n", str(n), "--per-col", "100",
                     "--dump-outputs", str(tmp_path)])
    assert j["metric"] == "lm_lsmr_outer_iterations_per_sec" and j["unit"] == "LM outer iterations/s" and j["dtype"] == "f64"
    assert j["higher_is_better"] is True and j["steps"] == 10 and j["repeats"] == 1
    assert j["value"] > 0 and j["ms_per_step"] == pytest.approx(1e3 / j["value"], rel=1e-9)
    assert j["roofline"] is None and j["cpu_baseline"] is None and j["parity_vs_cpu"] is None
    x, f = np.load(tmp_path / "minimizer.npy"), np.load(tmp_path / "residual.npy")
    ssr, counts = np.load(tmp_path / "ssr.npy"), np.load(tmp_path / "counts.npy")
    assert x.dtype == f.dtype == ssr.dtype == counts.dtype == np.float64
    assert x.shape == (n,) and f.shape == (m,) and counts.shape == (6,)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(f)) and 0 < counts[0] <= 10
    assert ssr[0] == pytest.approx(j["config"]["final_ssr"], rel=1e-15)
    assert float(np.sum(f * f)) == pytest.approx(ssr[0], rel=1e-9)
