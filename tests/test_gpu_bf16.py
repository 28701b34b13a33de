"""The bf16 MFMA mode (OPRL_PREC_BF16, include/oprl_amd.h) of the fused update kernels, through the C-ABI.

Two yardsticks per scenario (the scripted update sequences of tests/scenarios.py, i.e. of the golden
files):

* the EMULATION: the CPU oracle with both operands of every forward / backward GEMM rounded to bf16
  (``oracle.oprl_oracle.bf16_gemm``) — what the kernels claim to compute.  Differences are summation
  order plus the rare activation that lands on another side of a bf16 rounding boundary;
* the REFERENCE: the fp32 golden vectors generated from the reference itself — what the mode costs.
  bf16 inputs carry 8 mantissa bits (2^-9 = 2e-3 relative per operand), so this mode cannot meet the
  1e-4 gate of the fp32 parity mode (SURVEY.md section 0 measured 4.2e-3 on a critic forward); the
  gates below are what was measured on MI355X with head-room, the measured values are printed.

The probes (q, pi, log pi after the updates) are evaluated in fp32 on both sides — ``Module.__call__``
runs outside the fused kernels, from the fp32 packs — so they compare the WEIGHTS the updates left."""
import numpy as np
import pytest

from oracle import oprl_oracle as orc
from tests import hip_adapters as ha
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

# Measured on MI355X (tools/bf16_devs.py; the tests print theirs): vs the emulation <= 2.3e-6 on every
# key (outputs, parameters, Adam moments, step-1 gradients) — the gates are those of the fp32 parity tests;
# vs the fp32 reference vectors Q <= 8e-4, pi / log pi / parameter samples <= 5e-3 after 2..10 updates,
# single elements of the step-1 gradient samples up to 7e-2 of the largest element.
TOL_EMU_OUT, TOL_EMU_PARAM = 2e-5, 1e-4
# (parameter samples after k Adam steps sit within k * lr of each other: early Adam steps are sign-like, and
# bf16 decides the sign of the small gradients — 2e-2 of max|W| measured after 3 steps)
TOL_REF_OUT, TOL_REF_PARAM, TOL_REF_GRAD = 2e-2, 5e-2, 0.2


def _bf16_updates(cls, **emu_kw):
    """The oracle adapter with its update() under the bf16 GEMM emulation (probes stay fp32)."""
    class Emu(cls):
        def update(self, *a):
            with orc.bf16_gemm(**emu_kw):
                super().update(*a)
    return Emu


def _check(name, got, emu, gold, skip=(), emu_out=TOL_EMU_OUT, emu_param=TOL_EMU_PARAM, emu_actor_first=None, emu_moment=None):
    # The Adam moments (every scenario returns both optimizers' since round 6).  The CRITIC's are held at the parameters'
    # gate (`emu_moment`: TQC's own).  The ACTOR's: at `emu_actor_first` (default: the parameters' gate) after the first
    # update — where an actor-gradient scale error would show in full — and at 1e-3 of the largest moment afterwards: the
    # actor's gradient passes three bf16 GEMM chains (critic forward, critic backward, actor backward), a hidden activation
    # that lands on the other side of a bf16 rounding boundary than in the emulation flips one ReLU of one row, and a few
    # updates of that leave single moments 2.5e-4 apart (measured, DDPG after ten updates; the critic's moments and every
    # parameter sample stay below 1e-4)
    def is_actor_m(k): return ".m_actor." in k or ".v_actor." in k
    def is_critic_m(k): return ".m_critic." in k or ".v_critic." in k
    first_actor = {k: v for k, v in emu.items() if is_actor_m(k) and k.startswith("after1.")}
    late_actor = {k: v for k, v in emu.items() if is_actor_m(k) and not k.startswith("after1.")}
    critic_m = {k: v for k, v in emu.items() if is_critic_m(k)}
    rest = {k: v for k, v in emu.items() if not is_actor_m(k) and not is_critic_m(k)}
    we = sc.compare(got, rest, emu_out, skip=skip, param_tol=emu_param, moment_off_frac=None)
    for part, gate, what in ((first_actor, emu_actor_first if emu_actor_first is not None else emu_param, "the actor's Adam moments after the first update"),
                             (late_actor, max(1e-3, emu_moment or 0.0), "the actor's Adam moments after the later updates"),
                             (critic_m, emu_moment if emu_moment is not None else emu_param, "the critics' Adam moments")):
        if part:
            wl = sc.compare(got, part, emu_out, param_tol=gate, moment_off_frac=None)   # (not a parity mode: no element-count bound)
            print(f"\n[bf16] {name}: {what} vs the emulation: worst {wl[1]:.2e} ({wl[0]}), gate {gate:.0e}")
    # gradient-like keys (step-1 gradient samples, Adam moments): single elements, cancellation-prone
    def grad_like(k):
        return k.startswith(("g_critic_1", "g_actor_1")) or any(w in k for w in (".m_critic", ".v_critic", ".m_actor", ".v_actor"))
    wr = sc.compare(got, {k: v for k, v in gold.items() if not grad_like(k)}, TOL_REF_OUT, skip=skip,
                    param_tol=TOL_REF_PARAM)
    grads = {k: v for k, v in gold.items() if grad_like(k)}
    if grads:
        sc.compare(got, grads, TOL_REF_GRAD, param_tol=TOL_REF_GRAD, moment_off_frac=None)
    print(f"\n[bf16] {name}: worst rel. deviation vs bf16 emulation {we[1]:.2e} ({we[0]}), "
          f"vs fp32 reference vectors {wr[1]:.2e} ({wr[0]})")


def _ddpg_runs_whole_updates():
    """Does a bf16 DDPG learner at B = 256 take the whole-update form here (k_ddpg_chain<PrecBF16>: a chip that holds one
    update's workgroups)?  Its arithmetic differs from the phase launches' in two places the emulation follows
    (oracle.bf16_gemm(chain=True))."""
    import ctypes as C
    import torch as t
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.logging import NullLogger
    t.manual_seed(0)
    algo = DDPG(logger=NullLogger(), state_dim=24, action_dim=6, device="cuda", max_batch=256, precision="bf16").create()
    out = (C.c_int32 * 13)()
    assert algo.learner.lib.oprl_learner_debug_form(algo.learner.handle, 256, out) == 0
    return out[2] == 4


def test_ddpg_walker_b256_bf16():
    got = sc.ddpg_scenario(lambda *a: ha.HipDDPG(*a, precision="bf16"))

    def emulate(chain):
        class EmuD(_bf16_updates(sc.OracleDDPG, chain=chain)):
            def hook_step1(self):
                self._g = (self.o.last["g_critic"], self.o.last["g_actor"])
        return sc.ddpg_scenario(EmuD)
    emu = emulate(False)
    if _ddpg_runs_whole_updates():
        # the updates themselves ran as whole-update launches: their arithmetic (bf16_gemm(chain=True)); the step-1 gradient
        # samples come from a gradient-exporting twin learner (tests/hip_adapters.py), i.e. from the phase launches
        chain = emulate(True)
        emu = {k: (v if k.startswith("g_") else chain[k]) for k, v in emu.items()}
    _check("DDPG walker B=256, 10 updates", got, emu, sc.load_golden("ddpg_walker_b256"), skip=("y0", "q0"))


def test_td3_cheetah_b256_bf16():
    got = sc.td3_scenario(lambda *a: ha.HipTD3(*a, precision="bf16"))
    emu = sc.td3_scenario(_bf16_updates(sc.OracleTD3))
    _check("TD3 cheetah B=256, 3 updates", got, emu, sc.load_golden("td3_cheetah_b256"))


@pytest.mark.parametrize("env,B,seed,tune,steps,gold", [
    ("humanoid", 1024, 300, False, 2, "sac_humanoid_b1024"),
    ("walker", 256, 350, True, 3, "sac_walker_tune_b256"),
])
def test_sac_bf16(env, B, seed, tune, steps, gold):
    got = sc.sac_scenario(lambda *a: ha.HipSAC(*a, precision="bf16"), env, B, seed, tune, steps)
    emu = sc.sac_scenario(_bf16_updates(sc.OracleSAC), env, B, seed, tune, steps)
    # (the actor's first moments: 1.25e-4 at humanoid B = 1024 — 1024 rows x 3 chains of rounding boundaries; a scale error
    # would be O(1))
    _check(f"SAC {env} B={B}, {steps} updates", got, emu, sc.load_golden(gold), emu_actor_first=1e-3)


def test_tqc_walker_b256_bf16():
    """TQC: the five 512-wide quantile critics' hidden layers (97 % of the update's FLOPs) in bf16 through
    the layer-wise kernels; first layer, heads, quantile-Huber and the 256-wide actor in fp32."""
    got = sc.tqc_scenario(lambda *a: ha.HipTQC(*a, precision="bf16"))
    emu = sc.tqc_scenario(_bf16_updates(sc.OracleTQC, min_dim=512))
    # 1.3 M hidden activations per pass are rounded to bf16: a handful land on the other side of a rounding
    # boundary than in the emulation (summation order), the quantile-Huber indicator and Adam's sign-like
    # second step amplify that on single elements — measured 1.4e-4 on z, 2.2e-4 on one net's weight samples
    # after the second update (every other key <= 3e-5; tools/bf16_devs.py tqc)
    # ... and 3.4e-3 on single elements of the critics' first moments after the second update (m = 0.1 g2 + 0.09 g1: g2 is
    # the gradient at weights that already sit 2e-4 apart): the moment gate is 1e-2 (fp32 and x2 learners: 1e-6)
    _check("TQC walker B=256, 2 updates", got, emu, sc.load_golden("tqc_walker_b256"), skip=("qh.",),
           emu_out=1e-3, emu_param=2e-3, emu_actor_first=2e-3, emu_moment=1e-2)


def test_bf16_learner_actually_runs_the_bf16_kernels():
    """A bf16 learner must differ from the fp32 one (same inputs) by bf16-sized amounts — if the two
    agreed to 1e-6 the bf16 path would not be the one that ran."""
    import torch as t
    from oracle import fixtures as fx
    S, A, B = 24, 6, 256
    actor, critic = fx.make_net(1, fx.actor_dims(S, A)), fx.make_net(2, fx.critic_dims(S, A))
    a32, a16 = ha.HipDDPG(S, A, actor, critic), ha.HipDDPG(S, A, actor, critic, precision="bf16")
    for k in range(3):
        batch = fx.make_batch(10 + k, B, S, A)
        a32.update(*batch)
        a16.update(*batch)
    q32, y32 = a32.algo.learner.debug_q_y(B)
    q16, y16 = a16.algo.learner.debug_q_y(B)
    dq = sc.rel_dev(q16.cpu().numpy(), q32.cpu().numpy())
    assert 1e-5 < dq < 3e-2, dq
    assert bool(t.isfinite(a16.algo.critic._oprl_arena).all())
