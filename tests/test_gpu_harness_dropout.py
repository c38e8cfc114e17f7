"""GPU tier: scripts/harness.py `ilql` with the dropout flags at toy scale (the pattern of tests/test_gpu_harness.py): the flags reach the train
models, the step key comes from --seed, and the run trains and evaluates end to end."""
import importlib.util
import json
import os

import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_harness_ilql_with_dropout_flags(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec); spec.loader.exec_module(H)
    data = str(tmp_path / "d.jsonl")
    H.main(["gen-data", "--n-data", "24", "--out", data])
    common = ["ilql", "--train-data", data, "--epochs", "1", "--max-steps", "2", "--train-bsize", "8", "--max-length", "80", "--log-every", "1",
              "--policy-n-rollouts", "4", "--policy-bsize", "4", "--policy-max-input-length", "88", "--policy-max-output-length", "8", "--beta", "4"]
    capsys.readouterr()

    def losses(extra):
        H.main(common + ["--resid-pdrop", "0.1", "--attn-pdrop", "0.1", "--embd-pdrop", "0.1"] + extra)
        rows = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        got = [r["train"]["loss"] for r in rows if "train" in r]
        assert len(got) == 2 and any("eval" in r for r in rows), rows
        assert all(l == l and abs(l) < 1e6 for l in got), got
        return got

    # the Q heads start with a zero output layer, so the first loss cannot see the hidden states; the second one does (through the first update)
    a, b = losses(["--seed", "3"]), losses(["--seed", "4"])
    assert a[0] == b[0] and a[1] != b[1]       # the masks follow --seed
