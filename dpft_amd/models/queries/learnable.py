"""Learnable query reference points.

Mirror of ``src/dprt/models/queries/learnable.py`` (LearnableQueries :13-128): the parameter ``queries``
(prod(resolution), len(resolution)), the reference's exact initialisation sequence, and
``forward`` = repeat over the batch -> transformation.  Differences in *execution only*: on the GPU, three-dimensional
queries under no transformation or ``Spher2Cart`` (last dimension) come from one launch forward and one launch backward
(dpft_amd/csrc/queries.hip) instead of repeat + split + eight pointwise ops + cat and their backward chain; every other
configuration, and the CPU, runs the reference's torch ops.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence, Union

import torch
from torch import nn

from dpft_amd.models.utils.transformations import Spher2Cart, build_transformation


class _QueryCenterFn(torch.autograd.Function):
    """(Q,3) queries -> (B,Q,3) centres (dpft_query_center_fwd_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, queries, mode: int, B: int):
        from dpft_amd.hip.lib import lib, stream
        q = queries.detach().contiguous()
        center = torch.empty((B,) + tuple(q.shape), dtype=torch.float32, device=q.device)
        lib.call("dpft_query_center_fwd_f32", q.data_ptr(), mode, center.data_ptr(), B, q.shape[0], stream())
        ctx.save_for_backward(q)
        ctx.mode = mode
        return center

    @staticmethod
    def backward(ctx, dcenter):
        from dpft_amd.hip.lib import lib, stream
        (q,) = ctx.saved_tensors
        dcenter = dcenter.contiguous()
        dq = torch.empty_like(q)
        lib.call("dpft_query_center_bwd_f32", dcenter.data_ptr(), q.data_ptr(), ctx.mode, dq.data_ptr(), dcenter.shape[0],
                 q.shape[0], stream())
        return dq, None, None


class LearnableQueries(nn.Module):
    def __init__(self, resolution: List[int] = None, minimum: List[float] = None, maximum: List[float] = None,
                 q_init: str = None, transformation: nn.Module = None, **kwargs):
        super().__init__()
        self.resolution = resolution if resolution is not None else []
        self.minimum = minimum if minimum is not None else []
        self.maximum = maximum if maximum is not None else []
        self.q_init = q_init if q_init is not None else "uniform_"
        self.transformation = transformation if transformation is not None else nn.Identity()
        assert len(self.resolution) == len(self.minimum) == len(self.maximum)
        queries = torch.empty((torch.prod(torch.tensor(self.resolution)), len(self.resolution)))      # (N, dim)
        self.queries = nn.Parameter(queries)
        self.reset_parameters()

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "LearnableQueries":
        return cls(config["resolution"], config["minimum"], config["maximum"], config.get("q_init"),
                   transformation=build_transformation(config.get("transformation")))

    def reset_parameters(self) -> None:
        """learnable.py:95-101, op for op: the same seed gives the same bits."""
        if self.q_init == "uniform_":
            for i, (mi, ma) in enumerate(zip(self.minimum, self.maximum)):
                torch.nn.init.uniform_(self.queries[..., i], a=mi, b=ma)
        else:
            getattr(torch.nn.init, self.q_init)(self.queries)

    @staticmethod
    def _first(inp):
        # the batch size comes from the FIRST entry (learnable.py:85-93)
        if isinstance(inp, torch.Tensor):
            return inp
        if isinstance(inp, dict):
            return inp[list(inp.keys())[0]]
        return inp[0]

    def kernel_mode(self) -> Optional[int]:
        """The transformation code of dpft_query_center_*_f32 (include/dpft_hip.h: DPFT_QUERY_*), or None where the torch ops
        have to run."""
        q, t = self.queries, self.transformation
        if not q.is_cuda or q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != 3:
            return None
        if type(t) is nn.Identity:
            return 0
        if type(t) is Spher2Cart and t.dim in (-1, 2):
            return 2 if t.degrees else 1
        return None

    def __getstate__(self):          # the cached centres are rebuilt on demand (torch.save(model), deepcopy)
        st = self.__dict__.copy()
        st.pop("_centers", None)
        return st

    def forward(self, batch: Union[torch.Tensor, Sequence[torch.Tensor], Dict[str, torch.Tensor]]):
        B = self._first(batch).shape[0]
        if torch.is_grad_enabled():
            return OrderedDict({"center": self._centers_of(B)})
        # inference: the centres are a function of the parameter alone.  Kept until it changes -- an optimizer step, a
        # load_state_dict or an in-place edit bumps its version, kernels that write weights through raw pointers (the fused
        # AdamW, the EMA swap) bump hip.lib.weights_generation() -- and handed out read-only, like the static querent's.
        from dpft_amd.hip.lib import weights_generation
        q = self.queries
        key = (B, weights_generation(), q._version, q.data_ptr())
        kept = self.__dict__.get("_centers")
        if kept is None or kept[0] != key:
            kept = self.__dict__["_centers"] = (key, self._centers_of(B))
        return OrderedDict({"center": kept[1]})

    def _centers_of(self, B: int) -> torch.Tensor:
        mode = self.kernel_mode()
        if mode is not None:
            return _QueryCenterFn.apply(self.queries, mode, B)
        return self.transformation(self.queries.unsqueeze(0).repeat(B, 1, 1))       # learnable.py:122-126


def build_learnable_query(name: str, *args, **kwargs):
    return LearnableQueries.from_config(*args, **kwargs)
