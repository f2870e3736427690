"""The block schedules of the sequence-parallel forward (svi_hip.sequence_parallel.ulysses_blocks / gather_blocks / run_blocks), pinned
on the CPU: no GPU, no library.  The schedules take shard objects and a transport, so they are driven here with recording stand-ins
whose buffers are small real tensors.  The expected event lists are what a rank of a process group has to issue, in order: every
q | k exchange up front, V^T awaited first, per head group wait / attend / send the output, outputs awaited before the rest of the
block; gather mode: V^T leaves before the q | k projection, both gathers awaited before attention.  The in-process drivers
(forward_local[_pair]) run the same functions, so each of their shards must see the same list."""
from types import SimpleNamespace

import pytest
import torch

from svi_hip import sequence_parallel as sp

LS, DG, LD = 3, 4, 8                      # rows per shard, channels per head group, padded V^T row length
STAGES = ("block_qkv", "unpack_v", "attention", "block_rest", "block_v_rows", "block_qk_rows", "attention_rows", "block_rest_rows", "tea")


class Shard:
    """What the schedules touch of a SequenceShard: .dit.num_layers, .mode, .G, .buf and the stage methods (recorded, no arithmetic)."""

    def __init__(self, rank, P, G, mode, nb, log, gen):
        self.rank, self.G, self.mode, self.log = rank, G, mode, log
        self.dit = SimpleNamespace(num_layers=2)
        rnd = lambda *shape: torch.randn(shape, generator=gen)      # noqa: E731
        n, D = LS * nb * DG, P * G * DG
        if mode == "ulysses":
            self.buf = SimpleNamespace(qk_send=rnd(2, G, P, n), qk_recv=torch.zeros(2, G, P, n), vt_send=rnd(P, G * DG, LD), vt_recv=torch.zeros(P, G * DG, LD),
                                       o_send=rnd(G, P, n), o_recv=torch.zeros(G, P, n))
        else:
            self.buf = SimpleNamespace(k=rnd(LS, D), vt=rnd(D, LD), k_all=torch.zeros(P, LS, D), vt_all=torch.zeros(P, D, LD))

    def labels(self):
        """data pointer -> name of every tensor the schedule may hand to the transport: (receive side, send side) share a name."""
        b, out = self.buf, {}
        if self.mode == "ulysses":
            pairs = [("vt", b.vt_recv, b.vt_send)] + [(f"o{g}", b.o_recv[g], b.o_send[g]) for g in range(self.G)]
            pairs += [(f"{'qk'[o]}{g}", b.qk_recv[o, g], b.qk_send[o, g]) for o in (0, 1) for g in range(self.G)]
        else:
            pairs = [("vt", b.vt_all, b.vt), ("k", b.k_all, b.k)]
        for name, recv, send in pairs:
            out[(recv.data_ptr(), tuple(recv.shape))] = out[(send.data_ptr(), tuple(send.shape))] = name
        return out


for _name in STAGES:
    setattr(Shard, _name, lambda self, *args, _n=_name: self.log.append((self.rank, _n) + args))


class Recorder:
    """A transport that records every issue and every wait (rank None: seen by all shards of the process) and, given an inner
    transport, moves the data with it."""

    def __init__(self, shards, log, inner=None):
        self.shards, self.log, self.inner = shards, log, inner

    def _issue(self, op, recvs, sends):
        assert len(recvs) == len(sends) == len(self.shards)
        names = {sh.labels()[(t.data_ptr(), tuple(t.shape))] for sh, r, s in zip(self.shards, recvs, sends) for t in (r, s)}
        assert len(names) == 1, names                                # the same operand of every shard, receive and send side matched
        name = names.pop()
        self.log.append((None, op, name))
        if self.inner is not None:
            assert getattr(self.inner, op)(recvs, sends) is None
        return SimpleNamespace(wait=lambda: self.log.append((None, "wait", name)))

    def all_to_all(self, recvs, sends):
        return self._issue("all_to_all", recvs, sends)

    def all_gather(self, outs, mines):
        return self._issue("all_gather", outs, mines)


def ulysses_layer(layer, G):
    ev = [("block_qkv", layer), ("all_to_all", "vt")]
    ev += {1: [("all_to_all", "q0"), ("all_to_all", "k0")],
           2: [("all_to_all", "q0"), ("all_to_all", "k0"), ("all_to_all", "q1"), ("all_to_all", "k1")]}[G]
    ev += [("wait", "vt"), ("unpack_v",)]
    ev += [("wait", "q0"), ("wait", "k0"), ("attention", 0), ("all_to_all", "o0")]
    if G == 2:
        ev += [("wait", "q1"), ("wait", "k1"), ("attention", 1), ("all_to_all", "o1")]
    ev += {1: [("wait", "o0")], 2: [("wait", "o0"), ("wait", "o1")]}[G]
    return ev + [("block_rest", layer)]


def gather_layer(layer):
    return [("block_v_rows", layer), ("all_gather", "vt"), ("block_qk_rows", layer), ("all_gather", "k"), ("wait", "vt"), ("wait", "k"),
            ("attention_rows",), ("block_rest_rows", layer)]


def expected(mode, G, tea_mode, res):
    if tea_mode == 2:
        return [("tea", 2, res)]                                     # no block stage, no exchange
    blocks = gather_layer(0) + gather_layer(1) if mode == "gather" else ulysses_layer(0, G) + ulysses_layer(1, G)
    return blocks if tea_mode == 0 else [("tea", 0)] + blocks + [("tea", 1, res)]


def run(local_shards, world, G, mode, nb, tea_mode, move):
    """-> the shards, and per shard the events it saw (its own stage calls and every transport event)."""
    log, gen = [], torch.Generator().manual_seed(3)
    shards = [Shard(r, world, G, mode, nb, log, gen) for r in range(local_shards)]
    tr = Recorder(shards, log, sp.LocalTransport() if move else None)
    sp.run_blocks(shards, tr, tea_mode, [f"res{r}" for r in range(local_shards)] if tea_mode else None)
    return shards, [[e[1:] for e in log if e[0] in (None, r)] for r in range(local_shards)]


CASES = [("ulysses", 1, 1), ("ulysses", 2, 1), ("ulysses", 2, 2), ("gather", 1, 1)]       # mode, head groups, nb (2: the stacked pair)


@pytest.mark.parametrize("tea_mode", [0, 1, 2])
@pytest.mark.parametrize("mode,G,nb", CASES)
def test_one_rank_of_a_group_issues_the_pinned_sequence(mode, G, nb, tea_mode):
    _, (seen,) = run(1, 2, G, mode, nb, tea_mode, move=False)
    assert seen == expected(mode, G, tea_mode, "res0")


@pytest.mark.parametrize("tea_mode", [0, 1, 2])
@pytest.mark.parametrize("mode,G,nb", CASES)
def test_every_in_process_shard_sees_the_same_sequence(mode, G, nb, tea_mode):
    shards, seen = run(2, 2, G, mode, nb, tea_mode, move=True)
    for r in range(2):
        assert seen[r] == expected(mode, G, tea_mode, f"res{r}")
    if tea_mode == 2:
        return
    bufs = [sh.buf for sh in shards]                                 # and the copies put every piece where an all-to-all / all-gather puts it
    for j, b in enumerate(bufs):
        if mode == "gather":
            assert torch.equal(b.k_all, torch.stack([o.k for o in bufs])) and torch.equal(b.vt_all, torch.stack([o.vt for o in bufs]))
        else:
            assert torch.equal(b.vt_recv.flatten(1), sp.all_to_all_local([o.vt_send.flatten(1) for o in bufs])[j])
            assert torch.equal(b.qk_recv, sp.all_to_all_local([o.qk_send for o in bufs])[j])
            assert torch.equal(b.o_recv, sp.all_to_all_local([o.o_send for o in bufs])[j])


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_local_transport_is_the_exchange_algebra(P):
    gen = torch.Generator().manual_seed(P)
    tr = sp.LocalTransport()
    for shape in [(P, 5), (P, 3, 8)]:
        sends = [torch.randn(shape, generator=gen) for _ in range(P)]
        recvs = [torch.zeros(shape) for _ in range(P)]
        assert tr.all_to_all(recvs, sends) is None
        want = sp.all_to_all_local([s.flatten(1) for s in sends])
        assert all(torch.equal(r.flatten(1), w) for r, w in zip(recvs, want))
        mines = [torch.randn(shape[1:], generator=gen) for _ in range(P)]
        outs = [torch.zeros(shape) for _ in range(P)]
        assert tr.all_gather(outs, mines) is None
        assert all(torch.equal(o, torch.stack(mines)) for o in outs)
    rows = [torch.randn((4, 6), generator=gen) for _ in range(P)]
    assert torch.equal(tr.gather_rows(rows), torch.cat(rows))


def test_group_transport_issues_async_collectives_on_the_buffers_themselves(monkeypatch):
    """Not staged (anything but CUDA tensors over gloo): the collective gets the schedule's own buffers, async, and its handle comes back."""
    calls = []
    fake = SimpleNamespace(all_to_all_single=lambda recv, send, group=None, async_op=False: calls.append(("a2a", recv, send, group, async_op)) or "work",
                           all_gather_into_tensor=lambda out, mine, group=None, async_op=False: calls.append(("ag", out, mine, group, async_op)) or "work")
    monkeypatch.setattr(sp, "dist", fake)
    tr = sp.GroupTransport("grp")
    recv, send, mine = torch.zeros(2, 4), torch.ones(2, 4), torch.ones(4)
    assert tr.all_to_all([recv], [send]) == "work" and tr.all_gather([recv], [mine]) == "work"
    (op0, r0, s0, g0, a0), (op1, r1, s1, g1, a1) = calls
    assert (op0, g0, a0) == ("a2a", "grp", True) and r0 is recv and s0 is send
    assert (op1, g1, a1) == ("ag", "grp", True) and r1 is recv and s1 is mine
    sp._wait(None)                                                   # a synchronous exchange has nothing to wait for
    waited = []
    sp._wait(SimpleNamespace(wait=lambda: waited.append(1)))
    assert waited == [1]
