"""SHA-256 digests of what the engine hands to liblad_hip.so and of what comes back, for seeded inputs: the recorder behind
tests/test_launch_parent_gpu.py, which imports the cases from here.

    python tools/launch_digests.py [out.json]    (default: tests/golden/launch_parent.json)

_hip._lib is replaced by a recording proxy around the loaded CDLL.  For every call of a symbol of _hip.SIGNATURES it notes the
entry point's name, the value in every slot that is no pointer (as the slot's C type holds it) and, for a pointer slot, only whether
it is NULL.  Whatever the Python layer above looks like, it ends in lib().lad_...(...), so the same file records a commit and checks
a later one.  A case yields two digests: "calls", of the recorded sequence, and "results", of the bytes of what the case returns
(sweep_digests.sha).  Every case builds its own model (resnet_base widths, oracle.recipe.make_state(101)) on 100 x 44 windows.

The tool also prints, for every case, the entry points it reaches that its base case (train/default, predict/fp16) does not.  An
option stays in the lists below if it changes the recorded sequence; strip_block_fused and small_block_fused change nothing in
groups of CHUNK windows (engine._block_fits_lds) and are reached through the groups of CHUNK_LARGE."""
import contextlib
import ctypes
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sweep_digests import ROOT, sha  # noqa: E402  (puts the package, the repository root and tests/ on sys.path)

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_parent.json")
B_TRAIN = 4                    # the smallest batch every tile path accepts with margin
T_PREDICT, CHUNK = 300, 64     # more than one group, an even chunk, a shorter last group; fp16: the run path
T_LARGE, CHUNK_LARGE = 1100, 512   # groups large enough for the launches that keep images resident in LDS (engine._block_fits_lds)

# train/<option>: one changed option each
TRAIN_OPTIONS = {
    "default": {},
    "f32": dict(bf16x3=False),                 # every convolution on the exact-f32 MFMA
    "bf16x3": dict(f16x2=False),               # exact operands on three bf16 planes
    "no_f16x2_32": dict(f16x2_32=False),
    "no_relu_bits": dict(relu_bits=False),
    "no_virtual_a1": dict(virtual_a1=False),
    "fuse_bn_bwd": dict(fuse_bn_bwd=True),
    "no_fuse_bn_bwd_wgrad": dict(fuse_bn_bwd_wgrad=False),
    "no_fuse_s2_shortcut": dict(fuse_s2_shortcut=False),
    "no_s2_b3": dict(s2_b3=False),
    "no_stem_onepass": dict(stem_onepass=False),
    "overlap_wgrad": dict(overlap_wgrad=True),
    "no_bf16x3_32": dict(bf16x3_32=False),
    "no_fuse_bn_bwd_b3": dict(fuse_bn_bwd_b3=False),
    "no_fuse_s2_shortcut_wgrad": dict(fuse_s2_shortcut_wgrad=False),
    "no_defer_wgrad_sums": dict(defer_wgrad_sums=False),
}
# predict/fp16/<option>: the same for the switches of the sliding-window path
INFER_OPTIONS = {
    "no_stream": dict(stream=False),
    "no_stream_direct": dict(stream_direct=False),
    "no_stream_level2": dict(stream_level2=False),
    "no_stream_super": dict(stream_super=False),
    "no_tail_fused": dict(tail_fused=False),
    "no_strip2_resident": dict(strip2_resident=False),
    "no_strip_stem_shared": dict(strip_stem_shared=False),
    "no_f16_s2_shortcut_fused": dict(f16_s2_shortcut_fused=False),
    "windows_entry": dict(stream_level2=False, f16_s2_shortcut_fused=False),   # two switches: lad_f16_conv_s2_fwd_windows
}
# ... on T_LARGE windows in groups of CHUNK_LARGE
INFER_LARGE_OPTIONS = {
    "groups512": {},
    "groups512/no_strip_stem_shared": dict(strip_stem_shared=False),
    "groups512/no_tail_fused": dict(tail_fused=False),
}


# ---- the recording proxy ---------------------------------------------------------------------------------------------------------
def _is_pointer(argtype):
    return argtype is ctypes.c_void_p or argtype is ctypes.c_char_p or hasattr(argtype, "contents")


def _is_null(a):
    if a is None:
        return True
    if isinstance(a, int):
        return a == 0
    if isinstance(a, ctypes.c_void_p):
        return not a.value
    if isinstance(a, ctypes._Pointer):
        return not a
    return False                    # ctypes arrays, byref(...)


class Recorder:
    """Stands where _hip._lib stands: attribute access gives the CDLL's function behind a wrapper that notes the call."""

    def __init__(self, cdll, signatures):
        self._cdll, self._signatures, self.calls = cdll, signatures, []

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if name not in self._signatures:
            return fn
        argtypes = self._signatures[name][1]

        def call(*args):
            self.calls.append((name, tuple(("null" if _is_null(a) else "ptr") if _is_pointer(t) else t(getattr(a, "value", a)).value
                                           for t, a in zip(argtypes, args))))
            return fn(*args)
        setattr(self, name, call)
        return call


@contextlib.contextmanager
def recording():
    import _hip
    kept = _hip.lib()
    rec = _hip._lib = Recorder(kept._cdll if isinstance(kept, Recorder) else kept, _hip.SIGNATURES)
    try:
        yield rec
    finally:
        _hip._lib = kept


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def make_model(train):
    import torch

    import config
    from oracle import recipe
    cfg = config.MODEL_MAP["resnet_base"]
    with contextlib.redirect_stdout(io.StringIO()):
        model = cfg["model"](dropout_rate=0.5, linear_layer_size=cfg["linear_layer_size"], filter_sizes=cfg["filter_sizes"])
    full = model.state_dict()
    for k, v in recipe.make_state(101).items():
        full[k] = torch.from_numpy(v.copy())
    model.load_state_dict(full)
    model.set_device("cuda")
    model.train(train)
    return model


def _host(t):
    return t.detach().cpu().numpy().copy()


def train_step(options, accumulate=False):
    """One fused train step: forward with labels and "rng" dropout, backward(), clip_and_step().  -> probs, the flat gradient before
    the step, the flat parameters after it, the metric counters.  accumulate: without dropout, the step taken with the accumulation
    buffer (accumulate_grad), and eval_metrics of the probabilities as a fifth result."""
    import torch

    from oracle import recipe
    torch.manual_seed(1234)
    eng = make_model(True).engine
    for k, v in options.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    x = torch.from_numpy(recipe.make_features(77, B_TRAIN)).cuda()
    labels = torch.from_numpy(recipe.make_labels(4321, B_TRAIN)).cuda()
    probs = eng.forward(x, train=True, labels=labels, drop_masks=None if accumulate else "rng")
    extra = [_host(eng.eval_metrics(probs, labels))] if accumulate else []
    probs = _host(probs)
    eng.backward(None)
    grad = _host(eng.flat_grad())
    eng.clip_and_step(grad=eng.accumulate_grad(0.5) if accumulate else None)
    torch.cuda.synchronize()
    return [probs, grad, _host(eng.flat_param()), _host(eng.metrics())] + extra


class _EveryLabel(dict):
    """kernel_events with every label the engine uses: a label is in it as soon as it is asked for."""

    def __contains__(self, label):
        self.setdefault(label, [])
        return True


def predict(precision, options, events=False, T=T_PREDICT, chunk=CHUNK):
    """predict_windows over a (T, 44) feature matrix in groups of chunk.  -> the probabilities; events: the number of event
    pairs per label instead."""
    import torch

    from oracle import recipe
    eng = make_model(False).engine
    options = dict(options)
    stream = options.pop("stream", True)
    for k, v in options.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    if events:
        eng.kernel_events = _EveryLabel()
    feats = torch.from_numpy(np.ascontiguousarray(recipe.make_features(78, -(-T // 100)).reshape(-1, 44)[:T])).cuda()
    probs = eng.predict_windows(feats, chunk=chunk, precision=precision, stream=stream)
    torch.cuda.synchronize()
    if events:
        return repr(sorted((str(label), len(pairs)) for label, pairs in eng.kernel_events.items()))
    return _host(probs)


def cases():
    """{name: function without arguments that returns what is digested}."""
    out = {}
    for name, opts in TRAIN_OPTIONS.items():
        out[f"train/{name}"] = lambda o=opts: train_step(o)
    out["train/accumulate"] = lambda: train_step({}, accumulate=True)
    out["predict/fp32"] = lambda: predict("fp32", {})
    out["predict/fp16"] = lambda: predict("fp16", {})
    for name, opts in INFER_OPTIONS.items():
        out[f"predict/fp16/{name}"] = lambda o=opts: predict("fp16", o)
    for name, opts in INFER_LARGE_OPTIONS.items():
        out[f"predict/fp16/{name}"] = lambda o=opts: predict("fp16", o, T=T_LARGE, chunk=CHUNK_LARGE)
    out["events"] = lambda: predict("fp16", {}, events=True)
    out["events/groups512"] = lambda: predict("fp16", {}, events=True, T=T_LARGE, chunk=CHUNK_LARGE)
    return out


def run(fn):
    """-> ({"calls": digest, "results": digest}, the entry points reached)."""
    with recording() as rec:
        results = fn()
    return {"calls": sha(repr(rec.calls)), "results": sha(results)}, {name for name, _ in rec.calls}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    digests, reached = {}, {}
    for name, fn in cases().items():
        digests[name], reached[name] = run(fn)
    for name, names in reached.items():
        base = reached["train/default" if name.startswith("train/") else "predict/fp16"]   # (events: the same launches as its base)
        print(f"{name}: {len(names)} entry points; not in its base case: {sorted(names - base)}")
    print("reached by some case:", sorted(set().union(*reached.values())))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases -> {path}")


if __name__ == "__main__":
    main()
