"""GPU tier: `scripts/harness.py ppo --env twenty-questions` end to end at toy scale — the PPO script's loop (twenty_questions/ppo/train_ppo.py:
rollouts, the drop-the-last-turns rule, PPO data, steps, weights back) on the generic text path and on the device-resident loop."""
import importlib.util
import os

import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# random:small, not tiny: an oracle prompt of the default object list needs up to ~180 positions
BASE = ["ppo", "--env", "twenty-questions", "--model", "random:small", "--n-rollouts", "6", "--rollout-bsize", "4", "--train-bsize", "4", "--ppo-data-bsize", "4",
        "--max-input-length", "64", "--max-output-length", "6", "--tq-max-conversation-length", "3", "--tq-oracle-max-input-length", "224"]


def _harness():
    spec = importlib.util.spec_from_file_location("harness", os.path.join(ROOT, "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def test_harness_ppo_twenty_questions_host_path(capsys):
    _harness().main(BASE + ["--max-steps", "1"])
    out = capsys.readouterr().out
    assert out.count('"data_collection"') == 1 and '"train"' in out and '"eval"' in out and '"device_resident": true' not in out


def test_harness_ppo_twenty_questions_device_rollouts(capsys):
    H = _harness()
    H.main(BASE + ["--device-rollouts", "1", "--resident", "0", "--max-steps", "1"])
    H.main(BASE + ["--device-rollouts", "1", "--resident", "1", "--n-rounds", "2", "--max-steps", "2"])
    out = capsys.readouterr().out
    assert out.count('"data_collection"') == 3 and out.count('"device_resident": true') == 2 and '"eval"' in out
