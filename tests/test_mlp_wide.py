"""NN layer stacks wider than one CU's LDS: the streamed-weight MLP round and forward
pass (csrc/kernels/mlp.hip) against the CPU mirror, and the learner / engine on top."""
import functools
import json
import uuid

import pytest
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.io.synthetic import synth_batch, synth_json_records
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from omldm_amd.ops import native

SP = FeatureSpace(13, 0, 26, 1 << 14)
B, R, S, LR = 200, 64, 4, 0.05   # the last spoke holds 8 rows: a partial mini-batch
DACC_TOL = dict(rtol=2e-3, atol=2e-4)
STAT_TOL = dict(rtol=2e-3, atol=1e-2)
FWD_TOL = dict(rtol=1e-4, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _case(widths, task):
    """He-scaled weights (as the learner initialises), one NaN label inside a mini-batch
    and one mini-batch (rows 96..127) without any label."""
    g = torch.Generator().manual_seed(100 * len(widths) + task + widths[1])
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        parts += [torch.randn(b * a, generator=g) * (2.0 / a) ** 0.5,
                  torch.randn(b, generator=g) * 0.1]
    w = torch.cat(parts)
    x = torch.randn(B, widths[0], generator=g)
    if task == 0:
        y = x[:, 0] * 0.5 - x[:, 1]
    elif task == 1:
        y = torch.where(x[:, 0] + x[:, 2] > 0, 1.0, -1.0)
    else:
        y = (x @ torch.randn(widths[0], widths[-1], generator=g)).argmax(1).float()
    y[5] = float("nan")
    y[96:128] = float("nan")
    return w, x, y


@functools.lru_cache(maxsize=None)
def _reference(widths, task, act):
    """(dacc, stats, forward) of the fp32 CPU mirror, computed once per case."""
    w, x, y = _case(widths, task)
    d, s = torch.zeros_like(w), torch.zeros(8)
    D.mlp_round_reference(w, x, y, R, S, list(widths), task, LR, d, s, act)
    return d, s, D.mlp_forward_reference(w, x, list(widths), act)


def _gpu_round(cuda, widths, task, act):
    w, x, y = _case(widths, task)
    wd = w.to(cuda)
    d, s = torch.zeros_like(wd), torch.zeros(8, device=cuda)
    D.mlp_round(wd, x.to(cuda), y.to(cuda), R, S, list(widths), task, LR, d, s, act)
    out = D.mlp_forward(wd, x.to(cuda), list(widths), act)
    torch.cuda.synchronize()
    return d.cpu(), s.cpu(), out.cpu()


def _report(tag, got, ref):
    err = (got - ref).abs()
    print(f"{tag}: max|err| {float(err.max()):.3e}  max|ref| {float(ref.abs().max()):.3e}")


def _check(tag, got, ref):
    d, s, out = got
    d_ref, s_ref, o_ref = ref
    _report(f"{tag} dacc", d, d_ref)
    _report(f"{tag} stats", s[:4], s_ref[:4])
    _report(f"{tag} forward", out, o_ref)
    torch.testing.assert_close(d, d_ref, **DACC_TOL)
    torch.testing.assert_close(s[:4], s_ref[:4], **STAT_TOL)
    torch.testing.assert_close(out, o_ref, **FWD_TOL)


WIDE = [((13, 128, 128, 1), 1, 0),        # logistic, relu
        ((20, 260, 3), 2, 1),             # softmax, tanh; width no multiple of 16
        ((104, 256, 256, 1), 0, 2),       # regression, sigmoid
        ((13, 128, 128, 40), 2, 0),       # softmax past one 32-column tile
        ((13, 128, 128, 128, 1), 1, 3)]   # logistic, identity


@pytest.mark.gpu
@pytest.mark.parametrize("widths,task,act", WIDE)
def test_hip_mlp_wide_round_vs_reference(cuda, widths, task, act):
    """Stacks no fused kernel holds: dacc, stats[:4] and the forward pass agree with the CPU
    mirror within the bounds of test_hip_mlp_round_vs_reference (rtol 2e-3 / atol 2e-4,
    rtol 2e-3 / atol 1e-2, 1e-4)."""
    assert D.mlp_lds_bytes(list(widths)) > D.MLP_LDS_BUDGET   # the streamed form's ground
    assert D.mlp_fits(list(widths))
    _check(str(widths), _gpu_round(cuda, widths, task, act), _reference(widths, task, act))


@pytest.mark.gpu
@pytest.mark.parametrize("widths,task", [((13, 32, 32, 1), 1), ((7, 100, 3), 2)])
def test_hip_mlp_forced_stream_form_matches_fused(cuda, widths, task):
    """Where both forms take the stack, the streamed round (slab copy-in, training in
    place, subtraction) and the fused round each agree with the reference."""
    ref = _reference(widths, task, 0)
    lib = native.hip()
    _check(f"{widths} fused", _gpu_round(cuda, widths, task, 0), ref)
    prev = lib.omldm_mlp_form(-1)
    try:
        lib.omldm_mlp_form(4)
        _check(f"{widths} streamed", _gpu_round(cuda, widths, task, 0), ref)
    finally:
        lib.omldm_mlp_form(prev)


@pytest.mark.gpu
def test_hip_mlp_wide_bf16_vs_fp32_reference(cuda):
    """MLP_BF16 on the streamed form tracks the fp32 reference to bf16 rounding (the bounds
    of test_hip_mlp_bf16_matmul_vs_fp32_reference); integer operands are exact in bf16, so
    one streamed layer gives the fp32 result bit for bit.

    The round is compared under tanh: those bounds cover the rounding of quantities that
    are continuous in the operands, and ReLU's derivative is a step. With He-scaled
    128-wide layers some pre-activation always lies within bf16 rounding of zero (this
    case, fp32 mirror: unit 121 of the second layer at row 194, z = -1.0e-3 in fp32,
    +3.4e-3 with bf16 operands), and that row's whole gradient through the unit appears or
    vanishes: 6.7e-3 on weights of scale 8.3e-2 in the 8-row mini-batch (step lr/8). The
    forward pass is continuous under ReLU too and is checked with both."""
    widths, task = (13, 128, 128, 1), 1
    d_ref, _, o_ref = _reference(widths, task, 1)
    d, _, out = _gpu_round(cuda, widths, task, 1 | D.MLP_BF16)
    _report("bf16 tanh dacc", d, d_ref)
    _report("bf16 tanh forward", out, o_ref)
    scale = float(d_ref.abs().max())
    torch.testing.assert_close(d, d_ref, rtol=5e-2, atol=2e-2 * scale)
    torch.testing.assert_close(out, o_ref, rtol=3e-2, atol=3e-2 * float(o_ref.abs().max()))
    o_ref = _reference(widths, task, 0)[2]
    out = _gpu_round(cuda, widths, task, D.MLP_BF16)[2]
    _report("bf16 relu forward", out, o_ref)
    torch.testing.assert_close(out, o_ref, rtol=3e-2, atol=3e-2 * float(o_ref.abs().max()))
    wi = torch.randint(-3, 4, (13 * 32 + 32 + 32 * 1 + 1,)).float()
    xi = torch.randint(-3, 4, (64, 13)).float()
    lib = native.hip()
    prev = lib.omldm_mlp_form(-1)
    try:
        lib.omldm_mlp_form(4)
        o32 = D.mlp_forward(wi.to(cuda), xi.to(cuda), [13, 32, 1], 3).cpu()
        o16 = D.mlp_forward(wi.to(cuda), xi.to(cuda), [13, 32, 1], 3 | D.MLP_BF16).cpu()
    finally:
        lib.omldm_mlp_form(prev)
    assert torch.equal(o32, o16)
    assert torch.equal(o32, D.mlp_forward_reference(wi, xi, [13, 32, 1], 3))


@pytest.mark.gpu
def test_wide_nn_learner_on_gpu(cuda):
    hyper = {"hiddenLayers": [128, 128]}
    nn = make_learner("NN", hyper, SP, cuda)
    start = nn.state_vector().clone()
    for r in range(2):
        nn.fit(synth_batch(SP, 512, start=r * 512).to(cuda), RoundContext(spokes=4))
    assert not torch.equal(nn.state_vector(), start)
    t = synth_batch(SP, 96, start=10 ** 6).to(cuda)
    loss, score, n = nn.evaluate(t)
    assert n == 96 and torch.isfinite(loss) and nn.predict(t).shape == (96,)
    assert nn.running_totals()["fitted"] == 1024
    other = make_learner("NN", {**hyper, "seed": 3}, SP, cuda)
    assert not torch.equal(other.state_vector(), nn.state_vector())
    other.load_parameters(nn.parameters_map())
    torch.testing.assert_close(other.state_vector(), nn.state_vector(), rtol=0, atol=0)
    assert torch.equal(other.predict(t), nn.predict(t))


@pytest.mark.gpu
def test_wide_nn_engine_on_gpu(cuda):
    from omldm_amd.engine.job import Job
    from omldm_amd.io.transport import MemoryBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    name = uuid.uuid4().hex
    args = []
    for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
              "predictionsAddr", "performanceAddr"):
        args += [f"--{k}", f"memory://{name}"]
    cfg = JobConfig.from_args(args + ["--hashDim", str(SP.dim), "--timeout", "200",
                                      "--batchSize", "1000"])
    br = MemoryBroker.named(name)
    br.produce("requests", json.dumps({
        "id": 1, "request": "Create",
        "learner": {"name": "NN", "hyperParameters": {"hiddenLayers": [128, 128]}},
        "trainingConfiguration": {"protocol": "Synchronous"}}))
    for r in synth_json_records(2000, SP):
        br.produce("trainingData", r)
    br.produce("requests", json.dumps({"id": 1, "request": "Query", "requestId": 9}))
    job = Job(cfg, Comm(), cuda).run()
    assert job.terminated and job.pipes[1].learner.widths == [13, 128, 128, 1]
    assert job.pipes[1].learner.running_totals()["fitted"] > 0
    assert json.loads(br.records("performance")[-1])["statistics"][0]["fitted"] > 0
    assert any(json.loads(r).get("responseId") == 9 for r in br.records("responses"))


@pytest.mark.gpu
def test_nn_past_the_activation_budget_is_refused_at_construction(cuda):
    with pytest.raises(ValueError, match="activation budget"):
        make_learner("NN", {"hiddenLayers": [1024, 1024, 1024]}, SP, cuda)
    for widths in ([13, 128, 128, 1], [104, 128, 128, 1], [13, 256, 256, 1], [104, 256, 256, 1],
                   [13, 512, 1], [13, 128, 128, 128, 1], [13, 128, 128, 40]):
        assert 0 < D.mlp_stream_lds_bytes(widths) <= D.MLP_LDS_BUDGET, widths
