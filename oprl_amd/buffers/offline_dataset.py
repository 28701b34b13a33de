"""A fixed dataset into the HBM replay: offline RL (TD3+BC, algos/td3_bc.py).

``load_dataset`` reads an ``.npz`` with the usual D4RL key names; ``fill_replay`` cuts its rows into episodes and writes
them into an ``EpisodicReplayBuffer`` (or its n-step subclass), from where ``algo.update_from_buffer`` /
``trainers/offline_trainer.py`` train without an environment in the loop.  Everything here is host logic and works on
a ``device='cpu'`` buffer too.  (D4RL's own files are HDF5 behind a download; there is no reader for them here — the
datasets come from ``tools/make_offline_dataset.py``, or from whoever converts one to these keys.)

How the rows map onto the replay.  The replay stores an episode as states[e, 0 .. n] and per-step actions, rewards,
dones: the next state of step t IS states[e, t + 1], the observation of the following row.  So inside a piece only
``observations`` is read (``next_observations[t]`` is taken to be ``observations[t + 1]`` there, as it is in an
episode), and the piece's FINAL next state, the slot states[e, n] that ``add_transitions`` leaves stale, is written by
hand: ``next_observations`` of the last row where the dataset has that key; else the following row's observation for a
piece cut mid-episode; else, for a terminal row, the row's own observation (its value is multiplied by 1 - d = 0).  A
piece that ends in a timeout — or at the end of the file without a terminal — and has no ``next_observations`` has no
next state for its last row: that row is dropped."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np
import numpy.typing as npt
import torch as t

REQUIRED = ("observations", "actions", "rewards", "terminals")
OPTIONAL = ("timeouts", "next_observations")
NORM_EPS = 1e-3          # (x - mean) / (std + NORM_EPS), as in the authors' code


@dataclass
class OfflineData:
    observations: npt.NDArray             # [N, S]
    actions: npt.NDArray                  # [N, A]
    rewards: npt.NDArray                  # [N]
    terminals: npt.NDArray                # [N] bool
    timeouts: npt.NDArray | None = None   # [N] bool
    next_observations: npt.NDArray | None = None    # [N, S]

    def __len__(self) -> int:
        return len(self.observations)


@dataclass
class ObsNorm:
    """The observation statistics of a dataset (float64, ddof = 0, over all its rows)."""
    mean: npt.NDArray
    std: npt.NDArray

    def __call__(self, obs: npt.NDArray) -> npt.NDArray:
        """``(obs - mean) / (std + 1e-3)``, formed in float64, as float32."""
        return ((np.asarray(obs, dtype=np.float64) - self.mean) / (self.std + NORM_EPS)).astype(np.float32)

    def state_dict(self) -> dict:
        return {"mean": np.array(self.mean, dtype=np.float64), "std": np.array(self.std, dtype=np.float64)}


@dataclass
class Piece:
    start: int           # rows start .. stop - 1 of the dataset, one episode slot of the replay
    stop: int
    next_row: int        # the piece's final next state: observations[next_row] ...
    next_from_key: bool  # ... or next_observations[next_row]


def check_dataset(data: OfflineData) -> OfflineData:
    """Shapes and finiteness; returns the data with float64-free, contiguous arrays (float32 / bool)."""
    obs = np.asarray(data.observations)
    act = np.asarray(data.actions)
    if obs.ndim != 2 or act.ndim != 2 or obs.shape[0] < 1 or obs.shape[1] < 1 or act.shape[1] < 1:
        raise ValueError(f"dataset: observations [N, S] and actions [N, A] expected, got {obs.shape} and {act.shape}")
    N = obs.shape[0]
    if act.shape[0] != N:
        raise ValueError(f"dataset: {N} observations but {act.shape[0]} actions")

    def flat(x, name):
        x = np.asarray(x)
        if x.shape not in ((N,), (N, 1)):
            raise ValueError(f"dataset: {name} must be [{N}] (or [{N}, 1]), got {x.shape}")
        return x.reshape(N)

    rew = flat(data.rewards, "rewards")
    term = flat(data.terminals, "terminals")
    tout = flat(data.timeouts, "timeouts") if data.timeouts is not None else None
    nxt = np.asarray(data.next_observations) if data.next_observations is not None else None
    if nxt is not None and nxt.shape != obs.shape:
        raise ValueError(f"dataset: next_observations {nxt.shape} != observations {obs.shape}")
    for name, x in (("observations", obs), ("actions", act), ("rewards", rew), ("next_observations", nxt)):
        if x is not None and not np.all(np.isfinite(x)):
            raise ValueError(f"dataset: {name} holds a value that is not finite")
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)      # noqa: E731
    return OfflineData(f32(obs), f32(act), f32(rew), term.astype(bool), None if tout is None else tout.astype(bool),
                       None if nxt is None else f32(nxt))


def load_dataset(path) -> OfflineData:
    """An ``.npz`` with ``observations [N, S]``, ``actions [N, A]``, ``rewards [N]``, ``terminals [N]`` and, optionally,
    ``timeouts [N]`` and ``next_observations [N, S]`` (other keys are ignored)."""
    path = Path(path)
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in REQUIRED if k not in z.files]
        if missing:
            raise ValueError(f"{path}: missing the keys {missing} (has {sorted(z.files)})")
        kw = {k: z[k] for k in (*REQUIRED, *OPTIONAL) if k in z.files}
    return check_dataset(OfflineData(**kw))


def obs_statistics(data: OfflineData) -> ObsNorm:
    x = np.asarray(data.observations, dtype=np.float64)
    return ObsNorm(mean=x.mean(axis=0), std=x.std(axis=0, ddof=0))


def cut_pieces(data: OfflineData, max_len: int) -> tuple[list[Piece], int]:
    """The dataset's rows as pieces of at most ``max_len`` rows, and how many rows had to be dropped.  An episode ends
    after every ``terminals`` or ``timeouts`` row and at the end of the data; a longer one is cut into pieces."""
    if max_len < 1:
        raise ValueError(f"max_len={max_len}: at least one row per piece")
    N = len(data)
    has_next = data.next_observations is not None
    over = data.terminals.copy()
    if data.timeouts is not None:
        over |= data.timeouts
    over[N - 1] = True
    pieces: list[Piece] = []
    dropped = 0
    start = 0
    for end in np.flatnonzero(over):          # episode = rows start .. end
        end = int(end)
        for p0 in range(start, end + 1, max_len):
            p1 = min(p0 + max_len, end + 1)   # piece = rows p0 .. p1 - 1
            last = p1 - 1
            if has_next:
                pieces.append(Piece(p0, p1, last, True))
            elif last < end:                  # cut mid-episode: the following row's observation
                pieces.append(Piece(p0, p1, last + 1, False))
            elif data.terminals[last]:        # the value of s' is multiplied by 1 - d = 0
                pieces.append(Piece(p0, p1, last, False))
            else:                             # a timeout (or the end of the data): the last row has no next state
                dropped += 1
                if last > p0:
                    pieces.append(Piece(p0, last, last, False))
        start = end + 1
    return pieces, dropped


def fill_replay(buffer, data: OfflineData, normalize: bool = True) -> ObsNorm | None:
    """Write the dataset into ``buffer`` (created, nothing evicted: it raises ValueError if the pieces do not fit into
    the free episode slots behind the write pointer — it never wraps), one ``add_transitions(rows, episode_done=True)``
    per piece, then every piece's final next state.  With ``normalize`` the observations and next observations go
    through ``(x - mean) / (std + 1e-3)`` and the statistics come back as an ``ObsNorm`` (else None)."""
    buffer.check_created()
    data = check_dataset(data)
    S, A, L = buffer.state_dim, buffer.action_dim, buffer.max_episode_lenth
    if data.observations.shape[1] != S or data.actions.shape[1] != A:
        raise ValueError(f"dataset dims ({data.observations.shape[1]}, {data.actions.shape[1]}) != the buffer's ({S}, {A})")
    if getattr(buffer, "_lanes", None):
        raise ValueError("fill_replay: the buffer has open lanes (open_lanes); a dataset is written as whole episodes")
    pieces, _dropped = cut_pieces(data, L)
    E, p = buffer._max_episodes, buffer._ep_pointer
    # (every piece takes a slot, and closing the last one moves the pointer onto one more, which is evicted)
    if len(pieces) + 1 > E or any(buffer.ep_lens[(p + i) % E] > 0 for i in range(len(pieces) + 1)):
        raise ValueError(f"fill_replay: {len(pieces)} pieces (+ the open slot behind them) do not fit into the buffer's free "
                         f"episode slots ({E} slots of {L} steps); build it with buffer_size_transitions >= "
                         f"{(len(pieces) + 1) * L}")
    norm = obs_statistics(data) if normalize else None
    obs = norm(data.observations) if norm is not None else data.observations
    nxt = data.next_observations
    if nxt is not None and norm is not None:
        nxt = norm(nxt)
    rows = np.zeros((len(data), S + A + 2), dtype=np.float32)
    rows[:, :S] = obs
    rows[:, S:S + A] = data.actions
    rows[:, S + A] = data.rewards
    rows[:, S + A + 1] = data.terminals
    slots, lens, finals = [], [], []
    for pc in pieces:
        slots.append(buffer._ep_pointer)
        lens.append(pc.stop - pc.start)
        finals.append((nxt if pc.next_from_key else obs)[pc.next_row])
        buffer.add_transitions(rows[pc.start:pc.stop], episode_done=True)
    if pieces:
        states = buffer.states                # (flushes what is staged: the hand-written slots go in behind it)
        e_ix = t.as_tensor(slots, dtype=t.int64, device=states.device)
        n_ix = t.as_tensor(lens, dtype=t.int64, device=states.device)
        states[e_ix, n_ix] = t.from_numpy(np.stack(finals)).to(states.device)
    return norm
