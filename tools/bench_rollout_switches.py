"""bench.py with the Wordle rollout engine's two A/B switches preset (bench.py itself has no such options and stays as it is):

    python tools/bench_rollout_switches.py PIN_HEADER FUSED_TAIL [bench.py arguments]      # e.g.  1 0 --gpus 1 --steps 20 --warmup 5

Wraps `WordleRolloutEngine.__init__` so that `pin_header` / `fused_tail` default to the two 0 / 1 arguments, then runs bench.py as `__main__`.
Source of the "pin_header only" and "fused_tail only" rows of profiles/header_pin_fused_tail_ab.txt."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pin, fused = bool(int(sys.argv[1])), bool(int(sys.argv[2]))
import lmrl_gym_amd  # noqa: E402,F401
from lmrl_gym_amd import rollout  # noqa: E402

_init = rollout.WordleRolloutEngine.__init__


def _preset(self, *a, **kw):
    kw.setdefault("pin_header", pin)
    kw.setdefault("fused_tail", fused)
    _init(self, *a, **kw)


rollout.WordleRolloutEngine.__init__ = _preset
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[3:]
runpy.run_path(sys.argv[0], run_name="__main__")
