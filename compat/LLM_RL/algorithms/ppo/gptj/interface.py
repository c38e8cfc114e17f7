"""`LLM_RL.algorithms.ppo.gptj.interface` (reference: ppo/gptj/interface.py): the GPT-J policy on the fp32 HIP engine.
Inference only: the reference's `GPTJPPOTrain` / `GPTJPPOInference` have no counterpart yet (GPT-J train steps are not implemented).
The constructor takes a `GPTJEngineF32` instead of a flax TrainState; `act` / `set_params` keep the reference's signatures."""
from lmrl_gym_amd.gptj_f32_engine import GPTJConfig, GPTJEngineF32  # noqa: F401
from lmrl_gym_amd.policies import GPTJPPOPolicy  # noqa: F401
