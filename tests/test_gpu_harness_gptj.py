"""GPU tier: scripts/harness.py with a GPT-J policy (`--model-family gptj`): bc-eval runs on `GPTJEngineF32` through the text policy and logs an
eval summary; the device-resident rollout loop refuses the family before anything runs."""
import importlib.util
import json
import os

import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _harness():
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def test_bc_eval_runs_a_gptj_policy_and_device_rollouts_refuse_it(capsys):
    H = _harness()
    args = ["bc-eval", "--model", "random:gptj-tiny", "--model-family", "gptj", "--policy-n-rollouts", "4", "--policy-bsize", "2",
            "--policy-max-input-length", "88", "--policy-max-output-length", "8"]
    H.main(args)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    evals = [l["eval"] for l in lines if "eval" in l]
    assert len(evals) == 1 and set(evals[0]["reward"]) >= {"mean", "std", "min", "max"} and evals[0]["reward"]["mean"] <= 0.0
    with pytest.raises(SystemExit) as exc:
        H.main(args + ["--device-rollouts", "1"])
    assert exc.value.code not in (0, None) and "--model-family gptj is not available with --device-rollouts 1" in str(exc.value.code)


def test_maze_eval_runs_a_gptj_policy(capsys):
    H = _harness()
    H.main(["maze-eval", "--model", "random:gptj-tiny", "--model-family", "gptj", "--max-steps", "3", "--generation-bsize", "8", "--max-input-length", "160",
            "--max-output-length", "6"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    me = next(l["maze_eval"] for l in lines if "maze_eval" in l)
    assert me["n"] == 26 and 0.0 <= me["move_accuracy"] <= 100.0
