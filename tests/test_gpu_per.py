"""Prioritized replay's sum tree on the MI355X against tests/per_oracle.py: the tree through a script of writes,
recycled episodes (one evicted and refilled to the same length between two flushes), add_transitions blocks and
priority updates; the stratified sampler bit for bit, its frequencies on the 1000 x 1000 replay, its weights; the
duplicate-slot rule and p_max; a checkpoint round trip."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from tests import per_oracle as po

pytestmark = pytest.mark.gpu

S, A = 3, 1
ALPHA, EPS = 0.6, 1e-6


def make(E, L, **kw):
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    return PrioritizedEpisodicReplayBuffer(buffer_size_transitions=E * L, state_dim=S, action_dim=A,
                                           max_episode_lenth=L, device="cuda", alpha=ALPHA, eps=EPS, **kw).create()


class Tracked:
    """A buffer whose flushes and table uploads drive a TreeModel: the rows staged since the last flush and the
    table last uploaded are what the device's flush sees."""

    def __init__(self, E, L, seed=0):
        self.buf = b = make(E, L, seed=seed)
        self.model = po.TreeModel(E, L, ALPHA, EPS)
        self.model.enable([0] * E, 0)
        self.pending, self.uploaded = [], ([0] * E, 0)
        self.rng = np.random.default_rng(seed)
        flush, sync = b._flush, b._sync_lens

        def _flush():
            self.model.flush(self.pending, *self.uploaded)
            self.pending = []
            flush()

        def _sync_lens():
            sync()
            self.uploaded = (list(b.ep_lens), b.episodes_counter)
        b._flush, b._sync_lens = _flush, _sync_lens

    def row(self, done=False):
        r = self.rng.standard_normal(S + A + 2).astype(np.float32)
        r[S + A + 1] = float(done)
        return r

    def add(self, n, episode_done=False):
        for i in range(n):
            b = self.buf
            e = b._ep_pointer
            self.pending.append((e, b.ep_lens[e]))
            r = self.row(done=episode_done and i == n - 1)
            b.add_transition(r[:S], r[S:S + A], float(r[S + A]), bool(r[S + A + 1]), episode_done=episode_done and i == n - 1)

    def add_block(self, n, episode_done=False):
        b = self.buf
        e, l = b._ep_pointer, b.ep_lens[b._ep_pointer]
        self.pending += [(e, l + i) for i in range(n)]
        b.add_transitions(np.stack([self.row() for _ in range(n)]), episode_done=episode_done)

    def sync(self):
        self.buf._sync_lens()
        self.buf._flush()

    def update(self, slots, td):
        self.sync()
        self.model.update(list(slots), list(td))
        self.buf.update_priorities(t.as_tensor(np.asarray(slots, np.int32)), t.as_tensor(np.asarray(td, np.float32)))

    def sample_update(self, B):
        self.sync()
        self.buf.sample(B)
        slots = self.buf.last_slots.cpu().numpy()
        td = (self.rng.random(B) * 3).astype(np.float32)
        self.update(slots, td)
        return slots

    def check(self):
        self.sync()
        tree, pm = self.buf.tree()
        tree = tree.cpu().numpy()
        E, L = self.model.E, self.model.L
        leaves = tree[:E * L]
        assert np.array_equal(leaves, self.model.leaves), np.nonzero(leaves != self.model.leaves)[0][:10]
        assert np.array_equal(tree, po.build(leaves))                     # every node from its children, bit for bit
        assert pm == self.model.p_max
        b = self.buf
        live = np.zeros((E, L), bool)
        for e in range(b.episodes_counter):
            live[e, :b.ep_lens[e]] = True
        assert np.all(leaves.reshape(E, L)[~live] == 0) and np.all(leaves.reshape(E, L)[live] > 0)
        return tree


def script(tr: Tracked, E=7, L=50):
    """Ragged episodes, an in-progress tail, two trips round the ring, blocks and updates."""
    rng = np.random.default_rng(3)
    tr.add(12, episode_done=True)
    tr.add_block(30, episode_done=True)
    tr.add(5)
    tr.check()
    tr.sample_update(32)
    tr.check()
    for k in range(2 * E):
        n = int(rng.integers(3, L + 1))
        if k % 3 == 0:
            tr.add_block(n, episode_done=True)
        else:
            tr.add(n, episode_done=True)
        if k % 2 == 0:
            tr.sample_update(48)
        if k % 4 == 1:
            tr.check()
    # evict-and-refill to the same length between two flushes: the ring wraps onto the next slot (the wrap flushes,
    # then the slot is emptied) and a block of exactly its old length refills it before the next flush
    tr.sync()
    b = tr.buf
    nxt = (b._ep_pointer + 1) % b._max_episodes
    old = b.ep_lens[nxt]
    assert old > 0
    tr.add(4, episode_done=True)            # closes the current episode: the pointer moves onto nxt, which is evicted
    assert b._ep_pointer == nxt and b.ep_lens[nxt] == 0
    tr.add_block(old)
    assert b.ep_lens[nxt] == old
    tree = tr.check()
    assert np.all(tree[nxt * L:nxt * L + old] == tr.model.p_max)    # the refilled rows are new: p_max, not the old leaves
    tr.add(3)                               # an in-progress tail
    tr.sample_update(64)
    tr.check()


def test_tree_follows_the_model_through_a_script():
    tr = Tracked(7, 50)
    script(tr)
    # duplicates: the largest batch index sets the leaf; a dead slot is skipped; p_max grows
    b = tr.buf
    live = [e * 50 + t_ for e in range(b.episodes_counter) for t_ in range(b.ep_lens[e])]
    dead = next(e * 50 + b.ep_lens[e] for e in range(7) if b.ep_lens[e] < 50)
    s0, s1 = live[3], live[len(live) // 2]
    tr.update([s0, s1, s0, dead, s1, s0], [0.5, 7.0, 2.0, 50.0, 0.1, 30.0])
    tree = tr.check()
    assert tree[s0] == po.priority(30.0, ALPHA, EPS) and tree[s1] == po.priority(0.1, ALPHA, EPS) and tree[dead] == 0
    assert tr.model.p_max == po.priority(30.0, ALPHA, EPS)
    tr.update([s0], [1e-3])                                              # p_max does not shrink
    assert tr.buf.tree()[1] == po.priority(30.0, ALPHA, EPS)


def test_new_rows_take_p_max():
    tr = Tracked(7, 50)
    tr.add(10)
    tr.update(list(range(10)), [4.0] * 10)
    pm = po.priority(4.0, ALPHA, EPS)
    tr.add(2)
    leaves = tr.check()[:350]
    assert leaves[10] == pm and leaves[11] == pm and leaves[12] == 0


def test_sampler_is_bitwise_the_restatement_and_rows_match_storage():
    tr = Tracked(7, 50, seed=5)
    script(tr)
    b = tr.buf
    # zero priorities on a few live slots (through a checkpoint load): never drawn
    tr.sync()
    tree, pm = b.tree()
    leaves = tree[:350].clone()
    live = (leaves > 0).nonzero().flatten()
    zeroed = live[::5]
    leaves[zeroed] = 0
    from oprl_amd import _capi
    with _capi.on_device(b._dev):
        _capi.check(b._lib.oprl_replay_prio_load(b._handle, _capi.ptr(leaves), pm, _capi.current_stream()))
    tree = b.tree()[0].cpu().numpy()
    lv = tree[:350]
    assert np.array_equal(lv, leaves.cpu().numpy())
    st, ac, rw, dn = (b._tensors[k].cpu().numpy() for k in ("states", "actions", "rewards", "dones"))
    for B in (64, 1000, 37):
        counter = b._sample_counter
        s, a, r, d, s2 = b.sample(B)
        slots = b.last_slots.cpu().numpy()
        want = po.descend(tree, 350, B, b.seed, counter)
        assert slots.tolist() == want
        assert np.all(lv[slots] > 0) and not set(slots.tolist()) & set(zeroed.tolist())
        e, k = slots // 50, slots % 50
        assert np.array_equal(s.cpu().numpy(), st[e, k]) and np.array_equal(s2.cpu().numpy(), st[e, k + 1])
        assert np.array_equal(a.cpu().numpy(), ac[e, k]) and np.array_equal(r.cpu().numpy(), rw[e, k])
        assert np.array_equal(d.cpu().numpy(), dn[e, k])
        w = b.last_weights.cpu().numpy().astype(np.float64)
        ref = po.weights(lv, slots, b.beta(counter))
        assert np.max(np.abs(w - ref) / ref) < 1e-6


def test_sampler_frequencies_on_the_full_size_replay():
    """1000 x 1000 slots, ragged lengths, spread priorities; 1e6 draws binned by episode.  Chi-square with 999 degrees
    of freedom against p_e = (episode mass) / total must stay below df + 6 sqrt(2 df) (stratification only lowers it)."""
    E, L = 1000, 1000
    b = make(E, L, seed=9)
    rng = np.random.default_rng(0)
    lens = rng.integers(1, L + 1, size=E)
    b.ep_lens = [int(x) for x in lens]
    b.episodes_counter = E
    b._number_transitions = int(lens.sum())
    b._lens_dirty = True
    b._sync_lens()
    b._enable()
    leaves = t.as_tensor(rng.lognormal(0.0, 1.0, E * L).astype(np.float32), device="cuda")
    from oprl_amd import _capi
    _capi.check(b._lib.oprl_replay_prio_load(b._handle, _capi.ptr(leaves), 1.0, _capi.current_stream()))
    lv = b.tree()[0][:E * L].double()
    mass = lv.view(E, L).sum(1)
    counts = t.zeros(E, dtype=t.float64, device="cuda")
    D, B = 0, 50000
    for _ in range(20):
        b.sample(B)
        sl = b.last_slots.long()
        assert bool((lv[sl] > 0).all())
        counts += t.bincount(sl // L, minlength=E).double()
        D += B
    expect = D * mass / mass.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    df = E - 1
    assert chi2 < df + 6 * (2 * df) ** 0.5, chi2


def test_checkpoint_round_trip_is_bit_exact():
    tr = Tracked(7, 50, seed=2)
    script(tr)
    a = tr.buf
    sd = a.state_dict()
    b = make(7, 50)
    b.load_state_dict(sd)
    for name in ("states", "actions", "rewards", "dones"):
        assert t.equal(a._tensors[name], b._tensors[name])
    ta, pa = a.tree()
    tb, pb = b.tree()
    assert t.equal(ta, tb) and pa == pb
    td = t.rand(40, device="cuda")
    for buf in (a, b):
        buf.sample(40)
        buf.update_priorities(buf.last_slots, td)
    assert t.equal(a.last_slots, b.last_slots) and t.equal(a.last_weights, b.last_weights)
    assert t.equal(a.tree()[0], b.tree()[0])
    out = [buf.sample(40) for buf in (a, b)]
    assert all(t.equal(x, y) for x, y in zip(*out))
