"""`llm_rl_scripts.wordle.env.data` (reference: wordle/env/data.py:9-34) on the device episode loop."""
from lmrl_gym_amd.envs.wordle_policies import PolicyDataGenerator  # noqa: F401
