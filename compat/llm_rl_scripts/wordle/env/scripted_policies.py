"""`llm_rl_scripts.wordle.env.scripted_policies` (reference: wordle/env/scripted_policies.py:42-153) on the device policies."""
from lmrl_gym_amd.envs.wordle_policies import MixturePolicy, OptimalPolicy, RandomMixturePolicy, StartWordPolicy  # noqa: F401
