"""HBM-resident episodic replay buffer.

API, storage shapes and ring/eviction semantics of the reference
(/root/reference/src/oprl/buffers/episodic_buffer.py:13-140); the work is split
differently:

* index bookkeeping (episode ring pointer, per-episode lengths, live-transition
  count) is host logic and stays in Python ints, exactly as in the reference
  (:81-112), including its quirks: ``episodes_counter`` starts at 1, the slot
  the pointer advances onto is evicted immediately, ``add_episode`` with a
  terminal last row advances twice;
* data movement goes through liboprl_amd.so: ``add_transition`` stages the row
  in pinned host memory (``oprl_replay_write``) and rows reach HBM in one
  batched copy + scatter kernel at the next ``sample``/tensor access;
  ``sample`` is the gather kernel (``oprl_replay_sample``): uniform flat
  indices -> (episode, step) by binary search over cumulative episode ends ->
  one contiguous [s | s'] run + action + reward + done per sample, staged
  through LDS and written coalesced;
* several open episodes (extension): ``open_lanes(n)`` gives each of n lanes a slot of its
  own and ``add_step_rows`` writes one step of every lane — next states included — with one library call
  (``oprl_replay_write_rows``) and one ingest launch.

Storage is zero-filled instead of ``t.empty`` so the reference's reads of
never-written ``t+1`` slots are at least deterministic.
On ``device='cpu'`` the container and its bookkeeping work (host logic is
testable without a GPU) but ``sample`` raises: there is no CPU sampler."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import numpy.typing as npt
import torch as t

from oprl_amd import _capi
from oprl_amd.buffers.protocols import ReplayBufferProtocol

Transition = tuple[npt.NDArray, npt.NDArray, float, bool, npt.NDArray]
MAX_LANES = 256      # csrc/replay_internal.h kRowsMax: the records of one oprl_replay_write_rows call


@dataclass
class EpisodicReplayBuffer(ReplayBufferProtocol):
    buffer_size_transitions: int
    state_dim: int
    action_dim: int
    gamma: float = 0.99
    max_episode_lenth: int = 1000   # [sic] — the reference's spelling is the API
    episodes_counter: int = 1
    device: str = "cpu"
    seed: int = 0                   # device sampler key (Philox); extension

    _tensors: dict[str, t.Tensor] = field(init=False)
    _max_episodes: int = field(init=False)
    _ep_pointer: int = 0
    _number_transitions = 0
    _created: bool = False
    _lanes = None                   # open_lanes: the slot of every lane's running episode (None / empty: no lanes)

    def create(self) -> "EpisodicReplayBuffer":
        E = self._max_episodes = self.buffer_size_transitions // self.max_episode_lenth
        L, S, A = self.max_episode_lenth, self.state_dim, self.action_dim
        dev = t.device(self.device)
        self._tensors = {
            "actions": t.zeros((E, L, A), dtype=t.float32, device=dev),
            "rewards": t.zeros((E, L, 1), dtype=t.float32, device=dev),
            "dones": t.zeros((E, L, 1), dtype=t.float32, device=dev),
            "states": t.zeros((E, L + 1, S), dtype=t.float32, device=dev),
        }
        self.ep_lens = [0] * E
        self._handle = None
        self._lens_dirty = True
        self._sample_counter = 0
        self._lanes = []
        self._on_gpu = dev.type == "cuda"
        if self._on_gpu:
            self._dev = dev if dev.index is not None else t.device("cuda", t.cuda.current_device())
            lib = _capi.load()
            h = C.c_void_p()
            with _capi.on_device(self._dev):
                _capi.check(lib.oprl_replay_create(
                    E, L, S, A, _capi.ptr(self._tensors["states"]), _capi.ptr(self._tensors["actions"]),
                    _capi.ptr(self._tensors["rewards"]), _capi.ptr(self._tensors["dones"]), C.byref(h)),
                    "oprl_replay_create")
            self._handle = h
            self._lib = lib
        self._created = True
        return self

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                self._lib.oprl_replay_destroy(h)
            except Exception:
                pass
            self._handle = None

    def check_created(self) -> None:
        if not self._created:
            raise RuntimeError("Replay buffer has to be created with `.create()`.")

    # storage views (flush staged rows first so they are observable) -----------
    def _flush(self) -> None:
        if self._handle is not None:
            with _capi.on_device(self._dev):
                _capi.check(self._lib.oprl_replay_flush(self._handle, _capi.current_stream()),
                            "oprl_replay_flush")

    def _tensor(self, name: str) -> t.Tensor:
        self.check_created()
        self._flush()
        return self._tensors[name]

    @property
    def states(self) -> t.Tensor:
        return self._tensor("states")

    @property
    def actions(self) -> t.Tensor:
        return self._tensor("actions")

    @property
    def rewards(self) -> t.Tensor:
        return self._tensor("rewards")

    @property
    def dones(self) -> t.Tensor:
        return self._tensor("dones")

    # write path -----------------------------------------------------------------
    def add_transition(
        self,
        state: npt.NDArray,
        action: npt.NDArray,
        reward: float,
        done: bool,
        episode_done: bool | None = None,
    ) -> None:
        if self._lanes:
            self._refuse_with_lanes("add_transition")
        e, l = self._ep_pointer, self.ep_lens[self._ep_pointer]
        if l >= self.max_episode_lenth:
            raise IndexError(f"episode slot {e} is full ({l} steps, max_episode_lenth={self.max_episode_lenth})")
        s = np.ascontiguousarray(state, dtype=np.float32).reshape(self.state_dim)
        a = np.ascontiguousarray(action, dtype=np.float32).reshape(self.action_dim)  # f64 actions are cast
        eager = self._handle is not None and getattr(self, "eager_flush", False)
        if eager:
            pass        # (one library call below, once the episode table has this step in it)
        elif self._handle is not None:
            # (staging that fills up is flushed by the library: this buffer's device must be current then)
            with _capi.on_device(self._dev):
                _capi.check(self._lib.oprl_replay_write(
                    self._handle, e, l, s.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                    float(reward), float(done)), "oprl_replay_write")
        else:  # host container only (no GPU): plain row stores
            self._tensors["states"][e, l] = t.from_numpy(s)
            self._tensors["actions"][e, l] = t.from_numpy(a)
            self._tensors["rewards"][e, l] = float(reward)
            self._tensors["dones"][e, l] = float(done)
        self.ep_lens[e] += 1
        self._number_transitions = min(self._number_transitions + 1, self.buffer_size_transitions)
        self._touch_len(e)
        if episode_done:
            self._inc_episode()
        if eager:
            # the per-env-step caller (trainers/base_trainer.py): the row and the episode table go to HBM NOW — one
            # library call, one small launch that runs while the host walks on to the update call
            if self._lens_dirty or getattr(self, "_lens_np", None) is None:
                self._lens_np = np.asarray(self.ep_lens, dtype=np.int32).copy()
                self._lens_dirty = False
            with _capi.on_device(self._dev):
                _capi.check(self._lib.oprl_replay_write_flush(
                    self._handle, e, l, s.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), float(reward),
                    float(done), self._lens_np.ctypes.data_as(C.POINTER(C.c_int32)), self.episodes_counter,
                    _capi.current_stream()), "oprl_replay_write_flush")
            self._lens_touched = False

    def add_transitions(self, rows: npt.NDArray, episode_done: bool = False) -> None:
        """``len(rows)`` consecutive transitions of the episode being written, as float32 records
        ``[state (S) | action (A) | reward | done | ...]`` (extra columns ignored) — the bookkeeping of that many
        ``add_transition`` calls and ONE library call for the data (oprl_replay_write_block); with
        ``episode_done`` the episode is closed after the last one.  What the learner ranks of the distributed
        setup use to take in a whole actor episode (extension; the reference adds transitions one by one)."""
        if self._lanes:
            self._refuse_with_lanes("add_transitions")
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, S, A = len(rows), self.state_dim, self.action_dim
        if rows.ndim != 2 or rows.shape[1] < S + A + 2:
            raise ValueError(f"rows must be [n, >= {S + A + 2}] float32 records")
        e, l = self._ep_pointer, self.ep_lens[self._ep_pointer]
        if l + n > self.max_episode_lenth:
            raise IndexError(f"episode slot {e} would overflow ({l} + {n} steps, max_episode_lenth={self.max_episode_lenth})")
        if n:
            if self._handle is not None:
                with _capi.on_device(self._dev):
                    _capi.check(self._lib.oprl_replay_write_block(
                        self._handle, e, l, n, rows.ctypes.data_as(C.c_void_p), rows.shape[1],
                        _capi.current_stream()), "oprl_replay_write_block")
            else:
                self._tensors["states"][e, l:l + n] = t.from_numpy(rows[:, :S])
                self._tensors["actions"][e, l:l + n] = t.from_numpy(rows[:, S:S + A])
                self._tensors["rewards"][e, l:l + n, 0] = t.from_numpy(rows[:, S + A])
                self._tensors["dones"][e, l:l + n, 0] = t.from_numpy(rows[:, S + A + 1])
            self.ep_lens[e] += n
            self._number_transitions = min(self._number_transitions + n, self.buffer_size_transitions)
            self._touch_len(e)
        if episode_done:
            self._inc_episode()

    def _inc_episode(self) -> None:
        nxt = (self._ep_pointer + 1) % self._max_episodes
        if self.ep_lens[nxt] > 0:
            # the ring wraps onto a slot that holds data: rows staged for that slot and rows about to be
            # staged for it must not meet in one scatter launch (its blocks run in no particular order)
            self._flush()
        self._ep_pointer = (self._ep_pointer + 1) % self._max_episodes
        self.episodes_counter = min(self.episodes_counter + 1, self._max_episodes)
        self._number_transitions -= self.ep_lens[self._ep_pointer]
        self.ep_lens[self._ep_pointer] = 0
        self._touch_len(self._ep_pointer)

    def add_episode(self, episode: list[Transition]) -> None:
        if self._lanes:
            self._refuse_with_lanes("add_episode")
        for s, a, r, d, _ in episode:
            self.add_transition(s, a, r, d, episode_done=d)
        self._inc_episode()

    # several open episodes ---------------------------------
    def _refuse_with_lanes(self, what: str) -> None:
        raise RuntimeError(f"{what}: this buffer has {len(self._lanes)} open lanes (open_lanes); their episodes are "
                           "written by add_step_rows only")

    def open_lanes(self, n: int) -> None:
        """``n`` episodes open at once, one per lane: lane i takes slot i.  From here on the buffer is written by
        ``add_step_rows`` alone.  Needs an empty buffer; a second call with the same ``n`` does nothing."""
        self.check_created()
        E = self._max_episodes
        if isinstance(n, bool) or int(n) != n or not 1 <= n <= MAX_LANES or n > E - 1:
            raise ValueError(f"open_lanes({n!r}): expected 1 .. {min(MAX_LANES, E - 1)} (at most {MAX_LANES} lanes, and "
                             f"one of the {E} episode slots must stay free for the lane that closes)")
        n = int(n)
        if self._lanes:
            if len(self._lanes) == n:
                return
            raise RuntimeError(f"open_lanes({n}): {len(self._lanes)} lanes are open already")
        if self._number_transitions > 0 or any(self.ep_lens):
            raise RuntimeError(f"open_lanes({n}): the buffer already holds transitions")
        self._lanes = list(range(n))
        self._ep_pointer = n - 1
        self.episodes_counter = n
        self._lens_touched = True       # (the table's length changed)

    def _close_lane(self, i: int, held: set[int]) -> None:
        """Lane i's episode is over: the ring pointer moves on to the next slot no lane holds (lane i's own old slot
        counts as held until it has its new one), that slot is evicted and becomes lane i's."""
        E, p = self._max_episodes, self._ep_pointer
        while True:
            p = (p + 1) % E
            if p not in held:
                break
        self._ep_pointer = p
        self._number_transitions -= self.ep_lens[p]
        self.ep_lens[p] = 0
        self._touch_len(p)
        held.discard(self._lanes[i])
        held.add(p)
        self._lanes[i] = p
        self.episodes_counter = min(self.episodes_counter + 1, E)

    def add_step_rows(self, states: npt.NDArray, actions: npt.NDArray, rewards: npt.NDArray, dones: npt.NDArray,
                      next_states: npt.NDArray, episode_over: npt.NDArray) -> None:
        """One step of every lane: row i is the next step of lane i's episode and ``next_states[i]`` the state it led
        to, stored as ``states[slot, t + 1]`` — so the sampler finds s' behind the last stored step of a running
        episode and behind the last step of a truncated one.  Lanes whose ``episode_over`` is set move on to a fresh
        slot, in lane order.  ONE library call (oprl_replay_write_rows): the rows, the episode table and, on a
        prioritized replay, the leaves reach HBM with one ingest launch."""
        self.check_created()
        lanes = self._lanes
        if not lanes:
            raise RuntimeError("add_step_rows: no lanes are open (open_lanes)")
        N, S, A, L = len(lanes), self.state_dim, self.action_dim, self.max_episode_lenth
        s = np.ascontiguousarray(states, dtype=np.float32)
        a = np.ascontiguousarray(actions, dtype=np.float32)
        s2 = np.ascontiguousarray(next_states, dtype=np.float32)
        r = np.ascontiguousarray(rewards, dtype=np.float32).reshape(-1)
        d = np.ascontiguousarray(dones, dtype=np.float32).reshape(-1)
        over = np.asarray(episode_over, dtype=bool).reshape(-1)
        if s.shape != (N, S) or s2.shape != (N, S) or a.shape != (N, A) or not len(r) == len(d) == len(over) == N:
            raise ValueError(f"add_step_rows: expected states / next_states [{N}, {S}], actions [{N}, {A}] and {N} "
                             f"rewards, dones and episode_over; got {s.shape}, {s2.shape}, {a.shape}, {len(r)}, "
                             f"{len(d)}, {len(over)}")
        eps = np.asarray(lanes, dtype=np.int32)
        ts = np.asarray([self.ep_lens[e] for e in lanes], dtype=np.int32)
        if int(ts.max()) >= L:
            i = int(ts.argmax())
            raise IndexError(f"lane {i}: episode slot {lanes[i]} is full ({int(ts[i])} steps, max_episode_lenth={L})")
        # nothing can fail from here on
        for e in lanes:
            self.ep_lens[e] += 1
        mirror = getattr(self, "_lens_np", None)       # (_touch_len for all lanes at once)
        if mirror is None or len(mirror) != len(self.ep_lens):
            self._lens_dirty = True
        else:
            mirror[eps] = ts + 1
        self._number_transitions += N
        if over.any():
            held = set(lanes)
            for i in np.flatnonzero(over):
                self._close_lane(int(i), held)
        if self._handle is None:        # host container only (no GPU): plain row stores
            e_ix, t_ix = t.from_numpy(eps.astype(np.int64)), t.from_numpy(ts.astype(np.int64))
            self._tensors["states"][e_ix, t_ix] = t.from_numpy(s)
            self._tensors["states"][e_ix, t_ix + 1] = t.from_numpy(s2)
            self._tensors["actions"][e_ix, t_ix] = t.from_numpy(a)
            self._tensors["rewards"][e_ix, t_ix, 0] = t.from_numpy(r)
            self._tensors["dones"][e_ix, t_ix, 0] = t.from_numpy(d)
            return
        if self._lens_dirty or getattr(self, "_lens_np", None) is None:
            self._lens_np = np.asarray(self.ep_lens, dtype=np.int32).copy()
            self._lens_dirty = False
        i32, f32 = C.POINTER(C.c_int32), C.c_void_p
        with _capi.on_device(self._dev):
            _capi.check(self._lib.oprl_replay_write_rows(
                self._handle, N, eps.ctypes.data_as(i32), ts.ctypes.data_as(i32), s.ctypes.data_as(f32),
                a.ctypes.data_as(f32), r.ctypes.data_as(f32), d.ctypes.data_as(f32), s2.ctypes.data_as(f32),
                self._lens_np.ctypes.data_as(i32), self.episodes_counter, _capi.current_stream()),
                "oprl_replay_write_rows")
        self._lens_touched = False

    # read path ------------------------------------------------------------------
    def _touch_len(self, e: int) -> None:
        """ep_lens[e] changed through this class: keep the int32 mirror the library reads in step (one element — a
        mirror rebuilt from the list costs O(episodes) of python per env step, 20 us at a thousand episodes)."""
        mirror = getattr(self, "_lens_np", None)
        if mirror is None or len(mirror) != len(self.ep_lens):
            self._lens_dirty = True            # no mirror yet (or ep_lens was replaced): rebuild at the next sync
        else:
            mirror[e] = self.ep_lens[e]
            self._lens_touched = True

    def _sync_lens(self) -> None:
        if self._lens_dirty:                   # set by create / load_state_dict / whoever assigns ep_lens directly
            self._lens_np = np.asarray(self.ep_lens, dtype=np.int32).copy()
            self._lens_dirty = False
            self._lens_touched = True
        if getattr(self, "_lens_touched", False):
            n = self.episodes_counter
            with _capi.on_device(self._dev):
                _capi.check(self._lib.oprl_replay_set_lens(self._handle, self._lens_np.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                           _capi.current_stream()),
                            "oprl_replay_set_lens")
            self._lens_touched = False

    @property
    def handle(self):
        """C handle with the device-side episode table up to date (for step_n)."""
        self.check_created()
        if self._handle is None:
            raise RuntimeError("replay buffer is not on a GPU")
        self._sync_lens()
        return self._handle

    def _empty_rows(self, B: int):
        """The five outputs of a sampler call: (state, action, reward, done, next_state) for B rows, uninitialised."""
        S, A, dev = self.state_dim, self.action_dim, self._dev
        return (t.empty((B, S), dtype=t.float32, device=dev), t.empty((B, A), dtype=t.float32, device=dev),
                t.empty((B, 1), dtype=t.float32, device=dev), t.empty((B, 1), dtype=t.float32, device=dev),
                t.empty((B, S), dtype=t.float32, device=dev))

    def _refuse_empty(self, batch_size: int) -> None:
        """A batch of ``batch_size`` rows needs transitions to draw from (buffers/prior_buffer.py: in both sources)."""
        if self._number_transitions <= 0:
            raise ValueError("cannot sample from an empty replay buffer")

    def _sample(self, fn: str, batch_size: int, inds, return_indices: bool, extra: bool | None = None):
        """One call of the gather entry point ``fn`` — oprl_replay_sample, or with ``extra`` not None one of its
        n-step / hindsight / prior-data forms, which take one more optional int32[B] output — at this buffer's (seed, counter),
        which then moves on.  Returns ``(rows, (ep, step) | None, extra | None)``."""
        self.check_created()
        if self._handle is None:
            raise RuntimeError("sample() runs on the MI355X gather kernel; create the buffer with "
                               "device='cuda' (there is no CPU sampler)")
        self._refuse_empty(int(batch_size))
        self._sync_lens()
        B, dev = int(batch_size), self._dev
        rows = self._empty_rows(B)
        idx = None
        if inds is not None:
            idx = t.as_tensor(inds).to(device=dev, dtype=t.int64).contiguous()
            if idx.numel() != B:
                raise ValueError("inds must hold batch_size indices")
        ep = st = x = None
        if return_indices:
            ep = t.empty(B, dtype=t.int32, device=dev)
            st = t.empty(B, dtype=t.int32, device=dev)
        if extra:
            x = t.empty(B, dtype=t.int32, device=dev)
        ints = [_capi.ptr(ep), _capi.ptr(st)]
        if extra is not None:       # (oprl_replay_sample itself has no such argument)
            ints.append(_capi.ptr(x))
        with _capi.on_device(dev):
            _capi.check(getattr(self._lib, fn)(
                self._handle, B, _capi.ptr(idx), self.seed, self._sample_counter, *[_capi.ptr(v) for v in rows],
                *ints, _capi.current_stream()), fn)
        self._sample_counter += 1
        return rows, ((ep, st) if return_indices else None), x

    def sample(self, batch_size: int, inds: t.Tensor | npt.NDArray | None = None,
               return_indices: bool = False):
        """Uniform (with replacement) minibatch of live transitions, including the
        in-progress episode's tail — reference semantics (:123-133).  ``inds``:
        optional injected flat indices (what ``np.random.randint(0, len, B)``
        would return) for parity tests; None draws them on device."""
        rows, pair, _ = self._sample("oprl_replay_sample", batch_size, inds, return_indices)
        return (rows, pair) if return_indices else rows

    def _sync_sources(self) -> None:
        """The episode table of every storage a batch's rows come from, up to date on the device."""
        self._sync_lens()

    def returns_to_go(self, episodes, steps, gamma: float | None = None) -> t.Tensor:
        """The discounted return-to-go of the slots ``(episodes[i], steps[i])`` — what ``sample(return_indices=True)``
        gives — as a float32 device tensor [B] (oprl_replay_returns): the rewards from the slot to
        the episode's first done at or after it, or to its last stored step (no bootstrap at a truncation), discounted
        by ``gamma`` (default: the buffer's own).  A slot outside the storage gives 0."""
        self.check_created()
        if self._handle is None:
            raise RuntimeError("returns_to_go() runs on the MI355X returns kernel; create the buffer with "
                               "device='cuda' (there is no CPU path)")
        dev = self._dev
        ep = t.as_tensor(episodes).to(device=dev, dtype=t.int32).reshape(-1).contiguous()
        st = t.as_tensor(steps).to(device=dev, dtype=t.int32).reshape(-1).contiguous()
        if ep.numel() != st.numel():
            raise ValueError(f"{ep.numel()} episodes for {st.numel()} steps")
        B = ep.numel()
        self._sync_sources()
        out = t.empty(B, dtype=t.float32, device=dev)
        with _capi.on_device(dev):
            _capi.check(self._lib.oprl_replay_returns(
                self._handle, B, _capi.ptr(ep), _capi.ptr(st), float(self.gamma if gamma is None else gamma),
                _capi.ptr(out), _capi.current_stream()), "oprl_replay_returns")
        return out

    # ---- checkpoint ------------------------------------------------------
    def state_dict(self) -> dict:
        """Storage tensors (host copies) and the bookkeeping that decides where the next
        transition lands and which Philox counter the next sample() uses."""
        self._flush()
        return {
            "dims": (self.buffer_size_transitions, self.max_episode_lenth, self.state_dim, self.action_dim),
            "tensors": {k: v.detach().cpu().clone() for k, v in self._tensors.items()},
            "ep_lens": list(self.ep_lens), "episodes_counter": self.episodes_counter,
            "ep_pointer": self._ep_pointer, "number_transitions": self._number_transitions,
            "sample_counter": self._sample_counter, "seed": self.seed,
            "lanes": list(self._lanes or []),      # the slot of every lane's running episode (open_lanes)
        }

    def load_state_dict(self, sd: dict) -> None:
        self.check_created()
        dims = (self.buffer_size_transitions, self.max_episode_lenth, self.state_dim, self.action_dim)
        if tuple(sd["dims"]) != dims:
            raise ValueError(f"replay checkpoint dims {tuple(sd['dims'])} != {dims}")
        self._flush()
        for k, v in sd["tensors"].items():
            self._tensors[k].copy_(v.to(self._tensors[k].device))
        self.ep_lens = list(sd["ep_lens"])
        self.episodes_counter = int(sd["episodes_counter"])
        self._ep_pointer = int(sd["ep_pointer"])
        self._number_transitions = int(sd["number_transitions"])
        self._sample_counter = int(sd["sample_counter"])
        self.seed = int(sd["seed"])
        self._lanes = [int(e) for e in sd.get("lanes", [])]     # (absent in older checkpoints: no lanes)
        self._lens_dirty = True

    @property
    def last_episode_length(self) -> int:
        return self.ep_lens[self._ep_pointer]

    def __len__(self) -> int:
        return self._number_transitions
