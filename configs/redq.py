"""REDQ on the MI355X learner — the REDQ the reference lists on its roadmap; written like configs/sac.py.
Defaults: 10 critics, a minimum over 2 of them, 20 updates per environment step.

    python configs/redq.py --env walker-walk --device cuda [--seeds N]

The RLPD recipe (Ball et al. 2023: an ensemble at a high update-to-data ratio, LayerNorm critics, half of every batch
from a fixed dataset; DESIGN.md sections 10, 20 and 24):

    python configs/redq.py --layer-norm --prior-data D.npz --prior-share 0.5
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import LayerNormScript  # noqa: E402
from oprl.algos.redq import REDQ  # noqa: E402

script = LayerNormScript(REDQ, "REDQ", estimate_q_every=5000, log_every=1000)
# the names a reference-style script defines at module level
make_env, make_algo, make_replay_buffer, make_logger, config = (
    script.make_env, script.make_algo, script.make_replay_buffer, script.make_logger, script.config)

if __name__ == "__main__":
    script.run()
