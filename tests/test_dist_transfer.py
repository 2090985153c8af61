"""gkarray_amd.dist.exchange_streams over gloo with host-engine sets (world 2
and 3, launched as tests/test_dist.py launches its ranks): a rebalance to a
``balanced_assignment``, a swap between two ranks, a rank's own loop-back, and a
count mismatch that raises on the receiver without changing its set.  After
each, every stream of every rank is compared bit for bit with oracles moved the
same way in Python."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rollup_cases as R
from gk_oracle import OracleGK
from gkarray_amd import dist as gd
from test_dist import free_port

S, EPS = 12, 0.05


def rank_data(rank, case):
    """Values of rank `rank`'s S streams.  "rebalance": global stream g lives in
    slot g of rank g % world only (the worker blanks the rest)."""
    rng = np.random.default_rng(77 + rank)
    lens = rng.integers(0, 150, S)
    lens[rank] = 0
    return [rng.lognormal(0, 1, int(L)) for L in lens]


def owned(world, rank):
    return [g for g in range(S) if g % world == rank]


def lengths(world):
    """Length of global stream g (its owner's slot g)."""
    return [len(rank_data(g % world, "rebalance")[g]) for g in range(S)]


def plan(case, world, rank):
    """(send_ids, recv_ids, reset) of `rank`."""
    send = [[] for _ in range(world)]
    recv = [[] for _ in range(world)]
    reset = []
    if case == "rebalance":
        parts = [p.tolist() for p in gd.balanced_assignment(lengths(world), world)]
        for p in range(world):
            if p != rank:
                send[p] = [g for g in owned(world, rank) if g in parts[p]]
                recv[p] = [g for g in owned(world, p) if g in parts[rank]]
                reset += send[p]
    elif case == "swap":  # ranks 0 and 1 swap two streams; a third rank takes no part
        pair = {0: [2, 5], 1: [7, 3]}
        if rank in pair:
            send[1 - rank] = pair[rank]
            recv[1 - rank] = pair[rank]
    elif case == "loopback":  # every rank swaps two of its own streams and copies a third
        send[rank] = [4, 9, 6]
        recv[rank] = [9, 4, 0]
    elif case == "mismatch":  # rank 0 sends two streams, rank 1 lists one
        if rank == 0:
            send[1] = [2, 5]
        if rank == 1:
            recv[0] = [7]
    return send, recv, reset


def _worker(rank, world, port, case, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gkarray_amd import StreamSet
        import parity_util as U
        seqs = rank_data(rank, case)
        if case == "rebalance":
            seqs = [x if g in owned(world, rank) else np.zeros(0) for g, x in enumerate(seqs)]
        ss = StreamSet(S, EPS, device="cpu")
        U.ingest_np(ss, seqs)
        send, recv, reset = plan(case, world, rank)
        raised = None
        try:
            gd.exchange_streams(ss, [torch.tensor(x, dtype=torch.int32) for x in send],
                                [torch.tensor(x, dtype=torch.int64) for x in recv])
        except ValueError as e:
            raised = str(e)
        if reset:
            ss.reset_select(torch.tensor(reset, dtype=torch.int32))
        # the moved streams go on: 30 more values into every stream
        more = [np.random.default_rng(500 + 10 * rank + s).random(30) for s in range(S)]
        U.ingest_np(ss, more)
        q.put((rank, raised, R.snapshot(ss)))
    finally:
        dist.destroy_process_group()


def run(case, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def expected(case, world, refused=()):
    """Oracles of every rank's streams after the exchange, moved as the plan says."""
    orc = []
    for r in range(world):
        row = []
        for g, x in enumerate(rank_data(r, case)):
            o = OracleGK(EPS)
            if case != "rebalance" or g in owned(world, r):
                o.add_many(x)
            row.append(o)
        orc.append(row)
    old = copy.deepcopy(orc)
    for r in range(world):
        if r in refused:
            continue
        send_r, recv_r, _ = plan(case, world, r)
        for p in range(world):
            send_p = plan(case, world, p)[0]
            for src, dst in zip(send_p[r], recv_r[p]):
                orc[r][dst] = copy.deepcopy(old[p][src])
    for r in range(world):
        for g in plan(case, world, r)[2]:
            orc[r][g] = OracleGK(EPS)
        for s in range(S):
            orc[r][s].add_many(np.random.default_rng(500 + 10 * r + s).random(30))
    return orc


def check(results, orc, what):
    for rank, _, st in results:
        for s in range(S):
            R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_oracle(orc[rank][s]),
                            "%s: rank %d stream %d" % (what, rank, s))


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_rebalances_to_a_balanced_assignment(world):
    parts = [p.tolist() for p in gd.balanced_assignment(lengths(world), world)]
    assert any(set(parts[r]) != set(owned(world, r)) for r in range(world))  # (something moves)
    results = run("rebalance", world)
    assert all(raised is None for _, raised, _ in results)
    orc = expected("rebalance", world)
    check(results, orc, "rebalance")
    # every global stream now lives on the rank the assignment names, and only there
    for rank, _, st in results:
        for g in range(S):
            assert (int(st["n"][g]) > 30) == (g in parts[rank] and lengths(world)[g] > 0), (rank, g)


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_swaps_streams_between_two_ranks(world):
    results = run("swap", world)
    assert all(raised is None for _, raised, _ in results)
    check(results, expected("swap", world), "swap")


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_loops_back_to_the_sending_rank(world):
    results = run("loopback", world)
    assert all(raised is None for _, raised, _ in results)
    check(results, expected("loopback", world), "loopback")


def test_exchange_length_mismatch_raises_without_mutation():
    results = run("mismatch", 2)
    assert results[0][1] is None
    assert results[1][1] is not None and "sent 2 stream(s)" in results[1][1]
    check(results, expected("mismatch", 2, refused=(1,)), "mismatch")
