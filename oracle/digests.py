"""SHA-256 digests that pin this package to facts about the reference without storing any of it: the generator
(oracle/gen_golden.py reference_digests) hashes what the imported reference produces, the tests
(tests/test_host.py, tests/test_kradar_dataset.py) hash the same thing computed by this package and compare.
tests/golden/reference_digests.json holds the digests only."""
from __future__ import annotations

import functools
import hashlib
import json

import torch

CONFIG_SECTIONS = ("computing", "train", "model", "evaluate")


def sha256_json(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def config_digest(cfg: dict) -> str:
    """The sections of a config file that tests/test_host.py compares (weights names included)."""
    return sha256_json({k: cfg[k] for k in CONFIG_SECTIONS})


def tensor_digest(t: torch.Tensor):
    """[dtype, shape, sha256 of the bytes]: equal digests <=> torch.equal for tensors without NaNs or signed zeros."""
    t = t.detach().cpu().contiguous()
    return [str(t.dtype), list(t.shape), hashlib.sha256(t.numpy().tobytes()).hexdigest()]


def state_layout_digest(sd) -> str:
    """Ordered parameter / buffer names and shapes of a state dict."""
    return sha256_json([[k, list(v.shape)] for k, v in sd.items()])


def _encode(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, list):
        return [_encode(x) for x in v]
    if isinstance(v, tuple):
        return {"tuple": [_encode(x) for x in v]}
    if isinstance(v, (set, frozenset)):
        return {"set": sorted(_encode(x) for x in v)}
    if isinstance(v, dict) and all(isinstance(k, str) for k in v):
        return {"dict": [[k, _encode(x)] for k, x in v.items()]}
    if isinstance(v, functools.partial):
        return {"partial": [_encode(v.func), _encode(v.args), _encode(v.keywords)]}
    if callable(v) and getattr(v, "__name__", None):
        return {"global": [getattr(v, "__module__", None), getattr(v, "__qualname__", v.__name__)]}
    raise TypeError(f"module attribute of type {type(v).__name__} has no digest form")


def module_tree_digest(model: torch.nn.Module, skip=(), state=lambda m: m.__dict__) -> str:
    """Every module of ``model`` except the subtrees named in ``skip`` (named_modules order): class path, the attributes
    it adds to a bare nn.Module (``state(m)`` -- what pickling it writes), parameter and buffer names and shapes, child
    names.  That is what ``torch.save(model)`` records besides the tensor values."""
    base = set(torch.nn.Module().__dict__)
    rows = []
    for name, mod in model.named_modules():
        if any(name == s or name.startswith(s + ".") for s in skip):
            continue
        st = state(mod)
        rows.append([name, type(mod).__module__, type(mod).__qualname__,
                     [[k, _encode(v)] for k, v in st.items() if k not in base],
                     [[k, None if p is None else list(p.shape), None if p is None else p.requires_grad]
                      for k, p in mod._parameters.items()],
                     [[k, None if b is None else list(b.shape)] for k, b in mod._buffers.items()],
                     sorted(mod._non_persistent_buffers_set), list(mod._modules)])
    return sha256_json(rows)
