"""Shared by the tests of the serving plan's MLP and tree entries
(test_serving_plan_nonlinear_cpu.py, test_serving_plan_nonlinear.py): NN pipelines with
seeded random biases, Hoeffding trees written node by node, the reference prediction with
its near-tie mask, and the arena / mirror helpers.

tests/serving_plan_cases.py (``make_pipeline``, ``fill_random``) fills the preprocessors and
leaves NN and HT at their initial state; ``make`` below fills those two. The same seed gives
the same parameters on every device.

Reference = ``Pipeline.predict`` on the batch. A near-tie of an NN, taken from the
reference's own forward pass: ``|out_0|`` (±1 output) or the top-two gap (classes) at most
1e-3 · max(1, |top|). A tree's answer is compared on every row.
"""
import torch

from omldm_amd.ops import serving as S
from tests.serving_plan_cases import make_pipeline, payload

# name → (learner, hyper-parameters, preprocessors, options, seed). The seeds were chosen on
# the CPU so that the reference alone has at most MAX_TIES near-ties in the 40 points.
NN_CASES = {
    "nn_reg_relu": ("NN", {"task": "regression", "hiddenLayers": [8], "activation": "relu"},
                    [], {}, 501),
    "nn_bin_tanh_std": ("NN", {"hiddenLayers": [64, 3], "activation": "tanh"},
                        ["StandardScaler"], {}, 522),
    "nn_mc5_sigmoid_poly": ("NN", {"nClasses": 5, "hiddenLayers": [7, 9, 4],
                                   "activation": "sigmoid"}, ["PolynomialFeatures"], {}, 503),
    "nn_one_identity": ("NN", {"hiddenLayers": [1], "activation": "identity"}, [], {}, 504),
}
# tree → (hyper-parameters, preprocessors, shape)
HT_CASES = {
    "ht_fresh": ({"nClasses": 2}, [], "fresh"),
    "ht_complete63": ({"nClasses": 3}, [], "complete63"),
    "ht_chain_at_max_depth": ({"nClasses": 2, "maxDepth": 6}, [], "chain"),
    "ht_deeper_than_max_depth": ({"nClasses": 4, "maxDepth": 4}, [], "deeper"),
    "ht_1024_nodes_32_classes": ({"nClasses": 32, "maxNodes": 1024}, [], "big"),
    "ht_poly_high_features": ({"nClasses": 3}, ["PolynomialFeatures"], "heap15_high"),
    "ht_std": ({"nClasses": 2}, ["StandardScaler"], "heap15"),
    # 13 numerical features: PolynomialFeatures(2) makes 104, more than the wave's lanes —
    # the lazy stage (the products taken per node), behind a scaler
    "ht_std_poly_104_features": ({"nClasses": 3}, ["StandardScaler", "PolynomialFeatures"],
                                 "heap63_all"),
}
WIDE = ("ht_std_poly_104_features",)
HT_SEEDS = {name: 600 + i for i, name in enumerate(HT_CASES)}
CASES = list(NN_CASES) + list(HT_CASES)
# (learner, hyper-parameters, preprocessors): the wave cannot serve these
LEFT_DIRECT = {
    "hidden_65": ("NN", {"hiddenLayers": [65]}, []),
    "classes_65": ("NN", {"nClasses": 65, "hiddenLayers": [8]}, []),
    "bf16_matmul": ("NN", {"hiddenLayers": [8], "matmulDtype": "bf16"}, []),
    "nodes_1025": ("HT", {"nClasses": 2, "maxNodes": 1025}, []),
}


def space_of(name: str):
    """The feature space of a case: ``space_small`` (5 numerical + 3 categorical), or 13
    numerical + 3 categorical for the WIDE ones."""
    from omldm_amd.api.batch import FeatureSpace
    from tests.serving_plan_cases import space_small

    return FeatureSpace(13, 0, 3, 1 << 12, field_aware=True) if name in WIDE else \
        space_small(True)


def fill_nn(learner, seed: int) -> None:
    """Seeded random weights and biases, the weights wide enough (3 / sqrt(in)) that the
    answers of the saturating activations vary over the points."""
    g = torch.Generator().manual_seed(seed)
    flat = learner.flat.detach().cpu().clone()
    o = 0
    for a, b in zip(learner.widths[:-1], learner.widths[1:]):
        flat[o:o + a * b] = torch.randn(a * b, generator=g) * (3.0 / a ** 0.5)
        flat[o + a * b:o + a * b + b] = torch.randn(b, generator=g) * 0.5
        if learner.act_name == "sigmoid" and o:  # inputs in (0, 1): centre the unit on 1/2
            flat[o + a * b:o + a * b + b] -= 0.5 * flat[o:o + a * b].view(b, a).sum(1)
        o += a * b + b
    learner.flat.copy_(flat.to(learner.flat.device))


def set_tree(learner, feat, thr, left, right, cc) -> None:
    """Writes the first len(feat) nodes of the tree directly (``cc``: [n, C])."""
    n = len(feat)
    dev = learner.state.device
    for dst, src in ((learner.feat, feat), (learner.thr, thr), (learner.left, left),
                     (learner.right, right)):
        dst[:n] = torch.as_tensor(src, dtype=torch.float32).to(dev)
    learner.cc[:n] = torch.as_tensor(cc, dtype=torch.float32).to(dev)
    learner.nnodes.fill_(n)


def _counts(n: int, C: int, g) -> torch.Tensor:
    return torch.randint(0, 50, (n, C), generator=g).float()


def heap_tree(learner, n: int, feats: range, g) -> None:
    """A complete binary tree of n nodes in heap order (children 2i + 1, 2i + 2; n odd)."""
    inner = (n - 1) // 2
    feat = [-1.0] * n
    thr, left, right = [0.0] * n, [0.0] * n, [0.0] * n
    for i in range(inner):
        feat[i] = float(feats[int(torch.randint(0, len(feats), (1,), generator=g))])
        thr[i] = float(torch.randn(1, generator=g)) * 0.5
        left[i], right[i] = float(2 * i + 1), float(2 * i + 2)
    set_tree(learner, feat, thr, left, right, _counts(n, learner.Cn, g))


def chain_tree(learner, n_inner: int, g) -> None:
    """A right-leaning chain: inner node 2k (depth k) has the leaf 2k + 1 on its left and
    the next inner node 2k + 2 on its right; the last node, a leaf, is at depth n_inner."""
    n = 2 * n_inner + 1
    feat = [-1.0] * n
    thr, left, right = [0.0] * n, [0.0] * n, [0.0] * n
    for k in range(n_inner):
        i = 2 * k
        feat[i] = float(k % learner.d)
        thr[i] = -0.5
        left[i], right[i] = float(i + 1), float(i + 2)
    set_tree(learner, feat, thr, left, right, _counts(n, learner.Cn, g))


def fill_tree(pipe, shape: str, seed: int, first_point=None) -> None:
    g = torch.Generator().manual_seed(seed)
    L = pipe.learner
    if shape == "fresh":
        return
    if shape == "complete63":  # depth 5; the leaf of the first point: its top two counts equal
        heap_tree(L, 63, range(L.d), g)
        leaf = int(L._route(first_point.to(L.state.device))[0])
        assert 31 <= leaf < 63
        L.cc[leaf] = torch.tensor([3.0, 17.0, 17.0]).to(L.state.device)
    elif shape == "chain":     # the last leaf at exactly maxDepth
        chain_tree(L, L.depth, g)
    elif shape == "deeper":    # inner nodes down to maxDepth + 1: the walk ends on one
        chain_tree(L, L.depth + 2, g)
    elif shape == "big":       # 1023 of 1024 nodes, depth 9
        heap_tree(L, 1023, range(L.d), g)
    elif shape == "heap63_all":
        heap_tree(L, 63, range(L.d), g)
    elif shape == "heap15_high":
        heap_tree(L, 15, range(5, L.d), g)
    else:
        heap_tree(L, 15, range(L.d), g)


def make(pid: int, name: str, space, device, batch=None, seed_shift: int = 0):
    """The pipeline of case ``name`` with its seeded parameters (``batch``: the test's points,
    needed by the tree whose tie leaf is the first point's)."""
    if name in NN_CASES:
        learner, hyper, pres, opt, seed = NN_CASES[name]
        pipe = make_pipeline(pid, (learner, {**hyper, "seed": seed + seed_shift}, pres, opt),
                             space, device, seed + seed_shift)
        fill_nn(pipe.learner, seed + seed_shift)
        return pipe
    hyper, pres, shape = HT_CASES[name]
    seed = HT_SEEDS[name] + seed_shift
    pipe = make_pipeline(pid, ("HT", hyper, pres, {}), space, device, seed)
    first = None
    if shape == "complete63":
        first = pipe._pre(batch.slice(0, 1).to(pipe.device), False).num.float()
    fill_tree(pipe, shape, seed, first)
    return pipe


# one plan of old kinds (linear, MultiClassPA, K-means: the cases and seeds 100 + i / 300 + i
# of tests/serving_plan_cases.py at their indices there) between MLP and tree entries
OLD = ["svm_std", "mc3", "km3"]
MIXED = ["svm_std", "nn_reg_relu", "ht_complete63", "nn_mc5_sigmoid_poly", "mc3",
         "ht_1024_nodes_32_classes", "km3", "nn_bin_tanh_std", "ht_poly_high_features",
         "ht_deeper_than_max_depth", "nn_one_identity", "ht_std"]


def mixed(space, batch, device, shift: int) -> list:
    """The MIXED pipelines, ids 10 + i; ``shift`` 200: a second parameter set."""
    pipes = []
    for i, c in enumerate(MIXED):
        if c in OLD:
            pipes.append(make_pipeline(10 + i, c, space, device, 100 + i + shift))
        else:
            pipes.append(make(10 + i, c, space, device, batch, seed_shift=shift))
    return pipes


def make_direct(pid: int, name: str, space, device):
    learner, hyper, pres = LEFT_DIRECT[name]
    return make_pipeline(pid, (learner, hyper, pres, {}), space, device, 1)


def reference(pipe, batch):
    """(prediction [B], near-tie mask [B]) of the batched predict on the pipeline's device."""
    b = batch.to(pipe.device)
    pred = pipe.predict(b).float().cpu()
    tie = torch.zeros(b.B, dtype=torch.bool)
    L = pipe.learner
    if L.NAME == "NN" and L.task_id:
        out = L.forward(pipe._pre(b, False).num).float().cpu()
        if L.task_id == 1:
            s = out[:, 0]
            tie = s.abs() <= 1e-3 * torch.clamp(s.abs(), min=1.0)
        else:
            top = out.topk(2, dim=1).values
            tie = (top[:, 0] - top[:, 1]) <= 1e-3 * torch.clamp(top[:, 0].abs(), min=1.0)
    return pred, tie


def arena_of(plan, device="cpu") -> torch.Tensor:
    arena = torch.zeros(max(1, plan.arena_floats), dtype=torch.float32, device=device)
    plan.write(arena)
    return arena


def mirror(plan, arena, space, batch) -> torch.Tensor:
    """[B, n_out] answers of the CPU mirror."""
    rows = [S.cpu_serve_plan(plan.table, arena, space, *payload(batch, i))
            for i in range(batch.B)]
    return torch.tensor(rows, dtype=torch.float32)
