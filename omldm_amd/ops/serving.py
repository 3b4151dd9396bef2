"""Persistent low-latency predict server (csrc/kernels/serving.hip).

One resident wavefront polls a coherent pinned host mailbox; a request is a host write
+ sequence bump, the answer comes back through the same mailbox — no kernel launch or
stream synchronisation on the request path. The wave exits on ``stop()`` or after its
lifetime. It reads one of two weight banks (``w`` / ``w1``), chosen per request: a
publisher writes new models into the bank no request reads and switches requests over
once the copy is complete (engine/forecast_server.py), so an answer never mixes versions.

``PredictServer`` scores hashed-linear rows of one weight matrix. ``PlanServer`` runs the
same wave from a serving plan (``build_plan``): per pipeline its StandardScaler /
MinMaxScaler / PolynomialFeatures(2) stages, then a hashed-linear or dense ridge row, a
MultiClassPA argmax or a K-means argmin — and, with ``build_plan(..., nonlinear=True)``, a
small NN (its forward pass, one unit per lane) or a Hoeffding tree (its walk, through LDS) —
with the parameters in two fp32 arenas that the learners and preprocessors fill through
their ``serving_write``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from omldm_amd.api.batch import HashedBatch
from omldm_amd.ops import native
from omldm_amd.ops.native import check, ptr

SIGS = [
    ("omldm_mailbox_alloc", C.c_void_p, []),
    ("omldm_mailbox_free", None, [C.c_void_p]),
    ("omldm_serve_start", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_longlong, C.c_void_p]),
    ("omldm_serve_plan_start", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_longlong, C.c_void_p]),
    ("omldm_serve_request", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_void_p, C.c_longlong, C.c_int]),
    ("omldm_serve_stop", None, [C.c_void_p]),
    ("omldm_serve_alive", C.c_int, [C.c_void_p]),
    ("omldm_serve_exit_reason", C.c_int, [C.c_void_p]),
    ("omldm_bank_word_alloc", C.c_void_p, []),
    ("omldm_bank_word_free", None, [C.c_void_p]),
    ("omldm_bank_word_set", C.c_int, [C.c_void_p, C.c_uint, C.c_void_p]),
]


def _lib():
    lib = native.hip()
    if not hasattr(lib, "omldm_serve_start"):
        for name, res, args in SIGS:
            fn = getattr(lib.cdll, name)
            fn.restype, fn.argtypes = res, args
            setattr(lib, name, fn)
    return lib


class PredictServer:
    def __init__(self, w: torch.Tensor, dn: int, dc: int, bias: bool = True, cat_span: int = 0,
                 w1: torch.Tensor | None = None):
        assert w.is_cuda
        self.lib = _lib()
        self.W = w if w.dim() == 2 else w.unsqueeze(0)
        self.W1 = None if w1 is None else (w1 if w1.dim() == 2 else w1.unsqueeze(0))
        assert self.W1 is None or (self.W1.shape == self.W.shape and
                                   self.W1.stride() == self.W.stride() and
                                   self.W1.dtype == self.W.dtype)
        self.M, self.dim = int(self.W.shape[0]), int(self.W.shape[1])
        self.dn, self.dc, self.bias, self.cspan = dn, dc, bias, cat_span
        self.mb = self.lib.omldm_mailbox_alloc()
        if not self.mb:
            raise RuntimeError("hipHostMalloc(coherent) failed for the serving mailbox")
        # The resident wave must not block other work queued on the device: a blocking
        # stream (e.g. hipExtStreamCreateWithCUMask's) serialises with the legacy default
        # stream, and a normal-priority pool stream can share a hardware queue with the
        # training streams. Measured (scripts/diag_serve_queue.py): a high-priority,
        # non-blocking stream never delays work on other streams.
        self._raw_stream = None
        self.stream = torch.cuda.Stream(w.device, priority=-1)
        self.out = (C.c_float * self.M)()

    def start(self, lifetime_us: int = 10_000_000) -> None:
        check(self.lib.omldm_serve_start(ptr(self.W), ptr(self.W1),
                                         int(self.W.dtype == torch.bfloat16),
                                         self.W.stride(0), self.M, self.dn, self.dc, self.dim,
                                         int(self.bias), self.cspan, self.mb, int(lifetime_us),
                                         self.stream.cuda_stream), "omldm_serve_start")
        import time

        t = time.time()
        while not self.lib.omldm_serve_alive(self.mb):
            if time.time() - t > 10:
                raise RuntimeError("serving wave did not start")
            time.sleep(1e-4)

    def request_raw(self, num_ptr: int, cat_ptr: int, timeout_us: int = 1_000_000,
                    bank: int = 0) -> list[float]:
        rc = self.lib.omldm_serve_request(self.mb, num_ptr, self.dn, cat_ptr, self.dc, self.M,
                                          self.out, timeout_us, int(bank))
        if rc:
            raise TimeoutError("serving wave did not answer")
        return list(self.out)

    def request(self, point: HashedBatch, bank: int = 0) -> list[float]:
        """Scores of one point (row 0 of a host batch) against the M models."""
        num = point.num[0].float().contiguous()
        cat = point.cat[0].to(torch.int64)
        if point.cat_span:
            cat = cat & 0xFFFF
        cat = cat.to(torch.int32).contiguous()
        return self.request_raw(num.data_ptr(), cat.data_ptr(), bank=bank)

    def stop(self) -> None:
        self.lib.omldm_serve_stop(self.mb)
        self.stream.synchronize()

    def close(self) -> None:
        if self.mb:
            self.stop()
            self.lib.omldm_mailbox_free(self.mb)
            self.mb = None
        if getattr(self, "_raw_stream", None):
            native.hip().omldm_stream_destroy(self._raw_stream)
            self._raw_stream = None


# ------------------------------------------------------------------ plan-driven serving
# The layout of csrc/kernels/serve_plan.h (the kernel, its launcher's validation and the
# CPU mirror read the same table).
PLAN_WORDS = 128
PLAN_MAX_MODELS = 60
PLAN_MAX_STAGES = 4
PLAN_LANES = 64
PLAN_KINDS = {"linear": 0, "multiclass": 1, "kmeans": 2, "mlp": 4, "tree": 5}  # (3: none)
PLAN_NONLINEAR = ("mlp", "tree")   # served only by build_plan(..., nonlinear=True)
PLAN_MLP_MAX_LAYERS, PLAN_MLP_MAX_WIDTH = 4, 64
PLAN_TREE_MAX_NODES, PLAN_TREE_MAX_CLASSES = 1024, 32
PLAN_STAGES = {"affine": 0, "poly2": 1, "poly2_lazy": 2}
PLAN_BIAS, PLAN_SIGN, PLAN_DENSE = 1, 2, 4
PL_KIND, PL_OUT, PL_STAGES, PL_FLAGS, PL_OFF, PL_WIDTH, PL_K, PL_STAGE0, PL_PAIRS = \
    0, 1, 2, 3, 4, 5, 6, 8, 64
PL_AUX = 24  # mlp: L, act, task, w_0..w_L; tree: N, C, depth
PLAN_ERRORS = {-10: "shape", -11: "more than 64 lanes", -12: "stages", -13: "arena extent",
               -14: "output index", -15: "pair table"}


@dataclass
class ServingPlan:
    """What ``build_plan`` returns. ``table``: int32 [n, PLAN_WORDS], one entry per served
    pipeline; ``regions``: the arena layout — (writer, offset, floats), each writer (a
    learner or a preprocessor) filling its region through ``serving_write``; ``served``:
    (pipeline id, index into the wave's results); ``direct``: the pipelines left for
    one-row predicts."""

    table: np.ndarray
    arena_floats: int
    regions: list = field(default_factory=list)
    served: list = field(default_factory=list)
    direct: list = field(default_factory=list)

    @property
    def n_out(self) -> int:
        return len(self.served)

    def write(self, arena: torch.Tensor) -> None:
        """Every served pipeline's current parameters into ``arena`` (fp32, arena_floats
        long): device-to-device on the current stream, no host synchronisation."""
        for writer, off, n in self.regions:
            writer.serving_write(arena[off:off + n])


def _plan_entry(pipe, space, out: int, off: int, nonlinear: bool = False):
    """(entry words, regions, arena end) of one pipeline, or None when the wave cannot
    serve it: an unknown learner or preprocessor, more than PLAN_MAX_STAGES stages, or more
    than PLAN_LANES lanes (dense width after the stages + categorical fields + bias). An
    MLP or a tree (NN, HT) is an entry only with ``nonlinear``."""
    pres = list(pipe.preprocessors)
    if len(pres) > PLAN_MAX_STAGES:
        return None
    e = np.zeros(PLAN_WORDS, dtype=np.int32)
    regions, npairs, d = [], 0, space.dn
    lane_d = None  # the lane width in front of a lazy poly2 stage (else: d)
    for s, p in enumerate(pres):
        st = p.serving_stage(d) if hasattr(p, "serving_stage") else None
        if st is None:
            return None
        kind, floats = st
        w = PL_STAGE0 + 4 * s
        if kind == "affine":
            e[w:w + 4] = (PLAN_STAGES[kind], off, off + d, d)
            regions.append((p, off, floats))
            off += floats
        else:  # poly2: the static pair table, in PolynomialFeatures._index order
            pairs = p.pair_index(d, "cpu").tolist()
            if d + len(pairs) > PLAN_LANES or npairs + len(pairs) > PLAN_WORDS - PL_PAIRS:
                # too wide for the lanes or the pair table. A tree reads one feature per
                # node, so as the LAST stage in front of one the map is not laid out at all:
                # the wave takes a node's product from its two lanes (kPlanPoly2Lazy)
                ent = pipe.learner.serving_entry(d + len(pairs)) \
                    if hasattr(pipe.learner, "serving_entry") else None
                if not (nonlinear and s == len(pres) - 1 and ent is not None
                        and ent["kind"] == "tree" and 1 <= d <= PLAN_LANES):
                    return None
                e[w:w + 4] = (PLAN_STAGES["poly2_lazy"], 0, 0, d)
                lane_d = d
                d += len(pairs)
                continue
            e[w:w + 4] = (PLAN_STAGES[kind], npairs, 0, d)
            for a, b in pairs:
                e[PL_PAIRS + npairs] = int(a) | (int(b) << 8)
                npairs += 1
            d += len(pairs)
    ent = pipe.learner.serving_entry(d) if hasattr(pipe.learner, "serving_entry") else None
    if ent is None or (ent["kind"] in PLAN_NONLINEAR and not nonlinear):
        return None
    if ent["kind"] in PLAN_NONLINEAR:
        lanes = d if lane_d is None else lane_d
        if not _aux_fits(ent):
            return None
        e[PL_AUX:PL_AUX + len(ent["aux"])] = ent["aux"]
    elif ent["kind"] == "kmeans":
        lanes = d
    else:
        lanes = d + (0 if ent["dense"] else space.dc) + int(ent["bias"])
    if lanes > PLAN_LANES or lanes < 1:
        return None
    floats = int(ent["rows"]) * int(ent["width"])
    if off + floats >= 2 ** 31:
        return None
    e[PL_KIND], e[PL_OUT], e[PL_STAGES] = PLAN_KINDS[ent["kind"]], out, len(pres)
    e[PL_FLAGS] = (PLAN_BIAS if ent["bias"] else 0) | (PLAN_SIGN if ent["sign"] else 0) | \
        (PLAN_DENSE if ent["dense"] else 0)
    e[PL_OFF], e[PL_WIDTH], e[PL_K] = off, ent["width"], ent["rows"]
    regions.append((pipe.learner, off, floats))
    return e, regions, off + floats


def _aux_fits(ent) -> bool:
    """The limits plan_check puts on an mlp / tree entry (serve_plan.h)."""
    aux = [int(v) for v in ent["aux"]]
    if ent["kind"] == "mlp":
        L, widths = aux[0], aux[3:]
        return (1 <= L <= PLAN_MLP_MAX_LAYERS and len(widths) == L + 1 and 0 <= aux[1] <= 3
                and 0 <= aux[2] <= 2 and all(1 <= w <= PLAN_MLP_MAX_WIDTH for w in widths)
                and ent["width"] == sum(a * b + b for a, b in zip(widths[:-1], widths[1:])))
    N, C, depth = aux
    return (1 <= N <= PLAN_TREE_MAX_NODES and 2 <= C <= PLAN_TREE_MAX_CLASSES and depth >= 0
            and ent["width"] == N * (4 + C))


def build_plan(pipes, space, nonlinear: bool = False) -> ServingPlan:
    """The serving plan over ``pipes`` (objects with ``id``, ``preprocessors``, ``learner``):
    hashed-linear learners, ORR, MultiClassPA and K-means behind StandardScaler /
    MinMaxScaler / PolynomialFeatures(2) stages that fit the wave's limits are served, the
    first PLAN_MAX_MODELS of them; every other pipeline is left direct. ``nonlinear``: NN
    (≤ 4 layers of ≤ 64 units, fp32 matmul) and Hoeffding trees (≤ 1024 nodes, ≤ 32 classes)
    are served as well, as ``mlp`` / ``tree`` entries; a tree directly behind a
    PolynomialFeatures(2) too wide for the lanes takes it as a lazy stage. Pure Python."""
    entries, regions, served, direct, off = [], [], [], [], 0
    fits = space.dn + space.dc <= PLAN_LANES - 3  # the request line's payload
    for pipe in pipes:
        got = _plan_entry(pipe, space, len(served), off, nonlinear) \
            if fits and len(served) < PLAN_MAX_MODELS else None
        if got is None:
            direct.append(pipe)
            continue
        e, regs, off = got
        entries.append(e)
        regions += regs
        served.append((pipe.id, len(served)))
    table = np.stack(entries) if entries else np.zeros((0, PLAN_WORDS), dtype=np.int32)
    return ServingPlan(table, off, regions, served, direct)


def cpu_serve_plan(table: np.ndarray, arena: torch.Tensor, space, num, cat,
                   cat_span: int | None = None) -> list[float]:
    """One point against a plan and a CPU arena through the CPU mirror of the kernel
    (csrc/host/serve_plan_cpu.cpp): the Mailbox results, one per plan entry. ``num`` [dn]
    float32 and ``cat`` [dc] int32 are the request line's payload; ``cat_span`` -1: the
    payload carries raw 32-bit category tokens (default: the space's wire format). Raises
    on a plan the launcher would refuse."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    arena = arena.float().contiguous()
    num = np.ascontiguousarray(num, dtype=np.float32)
    cat = np.ascontiguousarray(cat, dtype=np.int32)
    out = np.zeros(PLAN_MAX_MODELS, dtype=np.float32)
    rc = native.host().omldm_cpu_serve_plan(
        table.ctypes.data, int(table.shape[0]), arena.data_ptr(), int(arena.numel()), space.dn,
        space.dc, space.cat_span if cat_span is None else int(cat_span), space.dim,
        num.ctypes.data, cat.ctypes.data, out.ctypes.data)
    if rc:
        raise ValueError(f"serving plan refused: {PLAN_ERRORS.get(rc, rc)} ({rc})")
    return out[: table.shape[0]].tolist()


class PlanServer(PredictServer):
    """The resident wave driven by a serving plan (serve_plan_kernel): the surface of
    ``PredictServer``, with ``arena0`` / ``arena1`` the two parameter banks (fp32, one
    layout) a request's ``bank`` selects. The results are final predictions.
    ``cat_span`` -1: requests carry raw 32-bit category tokens, hashed by the wave
    (``request_raw``); default: the space's wire format."""

    def __init__(self, table: np.ndarray, arena0: torch.Tensor, space,
                 arena1: torch.Tensor | None = None, cat_span: int | None = None):
        assert arena0.is_cuda and arena0.dtype == torch.float32 and arena0.is_contiguous()
        assert arena1 is None or (arena1.shape == arena0.shape and arena1.is_cuda and
                                  arena1.dtype == torch.float32 and arena1.is_contiguous())
        self.lib = _lib()
        # pinned (mapped) host memory: the launcher validates it, the wave reads it once
        self.table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).pin_memory()
        self.A0, self.A1 = arena0, arena1
        self.M = int(self.table.shape[0])
        self.dn, self.dc, self.dim = space.dn, space.dc, space.dim
        self.cspan = space.cat_span if cat_span is None else int(cat_span)
        self.mb = self.lib.omldm_mailbox_alloc()
        if not self.mb:
            raise RuntimeError("hipHostMalloc(coherent) failed for the serving mailbox")
        self._raw_stream = None
        self.stream = torch.cuda.Stream(arena0.device, priority=-1)  # see PredictServer
        self.out = (C.c_float * max(1, self.M))()

    def start(self, lifetime_us: int = 10_000_000) -> None:
        rc = self.lib.omldm_serve_plan_start(
            self.table.data_ptr(), self.M, ptr(self.A0), ptr(self.A1), int(self.A0.numel()),
            self.dn, self.dc, self.cspan, self.dim, self.mb, int(lifetime_us),
            self.stream.cuda_stream)
        if rc in PLAN_ERRORS:
            raise ValueError(f"serving plan refused: {PLAN_ERRORS[rc]} ({rc})")
        check(rc, "omldm_serve_plan_start")
        import time

        t = time.time()
        while not self.lib.omldm_serve_alive(self.mb):
            if time.time() - t > 10:
                raise RuntimeError("serving wave did not start")
            time.sleep(1e-4)
