"""Regenerates tests/golden/launch_plans.json: which library entry points every network calls, in order, with which arguments
(run from the repo root: `python tests/golden/make_launch_plans.py [out.json]`).

The GPU tests compare the kernels against torch within a tolerance, so they pass whichever path of a module's dispatch ran.  This
file pins the dispatch itself.  The networks run on CPU tensors with the library replaced by a recorder: `lib.load()` returns an
object whose every attribute appends (entry point, arguments) to a list, `fused.usable` / `fused32.usable` drop their `is_cuda`
term, and `F.conv2d` records itself and returns zeros, so no kernel and no half arithmetic of a convolution runs.  Per call the
integer and float arguments are kept, every pointer as 0 (null) or 1, and for the launches that write into a wider buffer the
destination's channel offset (f16: the last entry; fp32 `ss_op32_conv`: the storage offsets of x, out and res, the last three).
tests/test_launch_plan_cpu.py replays the same cases and compares.  The file holds a table of the distinct calls and, per case, the
indices into it.
"""
import ctypes as C
import inspect
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from strongsort_yolo_amd import fused, fused32, lib, nets           # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "launch_plans.json")
SWITCHED = ("yolov8n", "yolo11n")                                     # the detectors also recorded under each of SWITCHES
SWITCHES = (("HEAD", True), ("GROUP", False), ("BNECK", False), ("C3K2", False), ("POINTWISE", False))
DST_ARG = {"ss_op_pointwise_f16": 10, "ss_op_conv3x3_f16": 13, "ss_op_bottleneck_f16": 11, "ss_op_bias_act_place_f16": 8}
PLACERS = ("pointwise", "conv3x3", "bottleneck", "bottleneck_padded", "bias_act_place")


def _norm(a):
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return int(bool(a.value))
    if isinstance(a, (bool, int)):
        return int(a)
    if isinstance(a, float):
        return a
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, C.Array):
        if a._type_ is lib.ss_conv_desc:
            return [[int(bool(d.x)), int(bool(d.w)), int(bool(d.bias)), int(bool(d.out)), d.B, d.H, d.W, d.Cin, d.N, d.ksize, d.stride, d.act]
                    for d in a]
        return [int(bool(v)) if a._type_ is C.c_void_p else int(v) for v in a]
    raise TypeError(f"launch recorder: argument of type {type(a).__name__}")


class Recorder:
    """install(setattr) patches the package through `setattr(obj, name, value)` (pytest's monkeypatch.setattr, or plain setattr);
    .calls collects [entry point, [arguments]]."""

    def __init__(self):
        self.calls, self.base, self.extra = [], None, None

    def __getattr__(self, name):                                     # the stand-in for the loaded library
        def call(*args):
            rec = [_norm(a) for a in args]
            if name in DST_ARG:
                dst = args[DST_ARG[name]].value or 0
                rec.append(0 if self.base is None else (dst - self.base) // 2)
            if name == "ss_op32_conv":
                rec.extend(self.extra)
            self.calls.append([name, rec])
            return 1 if name.endswith(("_bands", "_bytes")) else 0
        return call

    def _placer(self, orig):
        names = list(inspect.signature(orig).parameters)

        def wrapper(*a, **kw):
            out = kw.get("out", a[names.index("out")] if len(a) > names.index("out") else None)
            old, self.base = self.base, (out.data_ptr() if out is not None else self.base)
            try:
                return orig(*a, **kw)
            finally:
                self.base = old
        return wrapper

    def _conv32(self, orig):
        def wrapper(x, mod, conv, act="silu", out=None, res=None):
            self.extra = [x.storage_offset(), 0 if out is None else out.storage_offset(), 0 if res is None else res.storage_offset()]
            return orig(x, mod, conv, act, out=out, res=res)
        return wrapper

    def _conv2d(self, x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        two = lambda v: [int(v), int(v)] if isinstance(v, int) else [int(t) for t in v]
        s, p, d = two(stride), two(padding), two(dilation)
        oh, ow = [(x.shape[2 + i] + 2 * p[i] - d[i] * (w.shape[2 + i] - 1) - 1) // s[i] + 1 for i in (0, 1)]
        self.calls.append(["conv2d", list(x.shape) + list(w.shape) + s + p + d + [int(groups), int(bias is not None)]])
        y = torch.zeros((x.shape[0], w.shape[0], oh, ow), dtype=x.dtype, device=x.device)
        return y.contiguous(memory_format=torch.channels_last) if x.is_contiguous(memory_format=torch.channels_last) else y

    def install(self, setattr_):
        setattr_(lib, "load", lambda: self)
        setattr_(fused, "_st", lambda x: None)
        setattr_(fused32, "_st", lambda x: None)
        setattr_(fused, "usable", lambda x: fused.ENABLED and x.dtype == torch.float16 and x.dim() == 4)
        setattr_(fused32, "usable", lambda x: fused32.ENABLED and isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4)
        for n in PLACERS:
            setattr_(fused, n, self._placer(getattr(fused, n)))
        setattr_(fused32, "conv", self._conv32(fused32.conv))
        setattr_(F, "conv2d", self._conv2d)


def cases():
    """(case name, network name, half?, (flag, value) or None)."""
    out = [(f"{n}/{p}", n, p == "f16", None) for n in list(nets.DETECTORS) + ["osnet"] for p in ("f16", "fp32")]
    out += [(f"{n}/f16/{k}={int(v)}", n, True, (k, v)) for n in SWITCHED for k, v in SWITCHES]
    return out


def run_case(name, half, switch, setattr_):
    """The calls of one forward pass.  `setattr_` as Recorder.install; it must undo what it set before the next case."""
    rec = Recorder()
    rec.install(setattr_)
    if switch is not None:
        setattr_(fused, switch[0], switch[1])
    net = nets.build_reid() if name == "osnet" else nets.build_detector(name)
    shape = (2, 3, 256, 128) if name == "osnet" else (2, 3, 128, 160)
    x = torch.zeros(shape).contiguous(memory_format=torch.channels_last)
    if half:
        net, x = net.half(), x.half()
    with torch.no_grad():
        net.to(memory_format=torch.channels_last)(x)
    return rec.calls


def pack(plans):
    """{case: calls} -> {"calls": [distinct calls], "plans": {case: [indices]}}."""
    table, index = [], {}
    packed = {}
    for case, calls in plans.items():
        packed[case] = [index.setdefault(json.dumps(c), len(index)) for c in calls]
    table = [json.loads(k) for k in index]
    return {"calls": table, "plans": packed}


def unpack(doc):
    return {case: [doc["calls"][i] for i in idx] for case, idx in doc["plans"].items()}


def dumps(doc):
    rows = ",\n".join(json.dumps(c, separators=(",", ":")) for c in doc["calls"])
    plans = ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in doc["plans"].items())
    return '{"calls":[\n' + rows + '\n],"plans":{\n' + plans + "\n}}\n"


class _Undo:
    def __init__(self):
        self.done = []

    def __call__(self, obj, name, value):
        self.done.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, old in reversed(self.done):
            setattr(obj, name, old)
        self.done = []


if __name__ == "__main__":
    plans, undo = {}, _Undo()
    for case, name, half, switch in cases():
        try:
            plans[case] = run_case(name, half, switch, undo)
        finally:
            undo.undo()
        print(case, len(plans[case]))
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as f:
        f.write(dumps(pack(plans)))
    print(path, os.path.getsize(path))
