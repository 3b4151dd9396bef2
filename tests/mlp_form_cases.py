"""Layer stacks that reach every kernel form of the NN learner (csrc/kernels/mlp.hip), with
the plan the launchers' routing query gives each: (round kernel, its waves, its LDS bytes,
forward kernel, its LDS bytes). tests/test_mlp_forms.py runs them on the GPU against the CPU
mirror at the sizes and bounds of tests/test_mlp_wide.py; tests/test_mlp_forms_cpu.py holds
the routing to these expectations without a device."""
from omldm_amd.ops.dense import MLP_BF16

RELU, TANH, SIGMOID, IDENTITY = 0, 1, 2, 3
REGRESSION, LOGISTIC, SOFTMAX = 0, 1, 2

# (widths, task, act, plan under the default form, what the case is there for)
FORM_CASES = [
    ((13, 32, 20), SOFTMAX, RELU, ("fused32", 4, 32640, "fused32", 32640),
     "v1 round and fused forward, output past one 16-column tile"),
    ((70, 32, 17), SOFTMAX, TANH, ("fused32", 4, 65408, "fused32", 65408),
     "v1, synchronous staging (padded input 96 > 64), K = 17"),
    ((70, 32, 3), SOFTMAX, SIGMOID, ("fused16", 16, 63760, "fused32", 65408),
     "v2, synchronous staging (padded input 80 > 64)"),
    ((96, 96, 96, 1), LOGISTIC, RELU, ("fused32", 4, 159232, "fused32", 159232),
     "output width 1 on v1: the 16-padded layout (164368 B) is past the LDS, the 32-padded "
     "one is not; synchronous staging"),
    ((32, 64, 160, 1), REGRESSION, IDENTITY, ("fused32", 4, 155776, "fused32", 155776),
     "the same edge (16-padded layout 165136 B) with the prefetch staging"),
]

# one stack under each fused form: (widths, task, act, {form: plan})
FORCED_CASE = ((13, 32, 32, 1), LOGISTIC, RELU,
               {0: ("fused32", 4, 41984, "fused32", 41984),
                3: ("fused16", 16, 38416, "fused32", 41984),
                4: ("stream", 16, 24000, "stream", 14336)})

# v1's bf16 operand path (the round under tanh: tests/test_mlp_forms.py says why)
BF16_CASE = ((13, 32, 20), SOFTMAX, TANH | MLP_BF16, FORM_CASES[0][3])

# the stacks of tests/test_mlp_wide.py (WIDE, in its order): streamed round and forward
WIDE_PLANS = [("stream", 16, 73920, "stream", 38912),
              ("stream", 16, 81664, "stream", 42496),
              ("stream", 16, 152768, "stream", 83968),
              ("stream", 16, 78144, "stream", 43008),
              ("stream", 16, 91328, "stream", 55808)]

ALL_PLANS = {("fused32", "fused32"), ("fused16", "fused32"), ("stream", "stream")}
