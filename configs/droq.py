"""DroQ on the MI355X learner (Hiraoka et al., ICLR 2022: dropout Q-functions) — written like configs/redq.py.
Defaults: 2 critics, both in the minimum, 20 updates per environment step, LayerNorm critics with dropout at rate 0.01
(Linear -> Dropout -> LayerNorm -> ReLU; DESIGN.md sections 10, 24 and 26).

    python configs/droq.py --env walker-walk --device cuda [--dropout RATE]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import LayerNormScript, droq_kwargs  # noqa: E402
from oprl.algos.droq import DroQ  # noqa: E402

script = LayerNormScript(DroQ, "DroQ", estimate_q_every=5000, log_every=1000, algo_kwargs=droq_kwargs, recipe=True)
# the names a reference-style script defines at module level
make_env, make_algo, make_replay_buffer, make_logger, config = (
    script.make_env, script.make_algo, script.make_replay_buffer, script.make_logger, script.config)

if __name__ == "__main__":
    script.run()
