"""nip_amd -- MI355X-native forward-backward join-tree engine for NIP's DBNs.

Python mirror of the reference's top-level interface for this path
(src/nip.h): ``parse_model`` / ``model_variable`` / ``forward_backward_inference``
/ ``em_learn``-pieces, batched over sequences and backed by the gfx950 C-ABI
library ``_lib/libnip_amd.so`` (include/nip_amd.h).  The library is loaded
through ctypes with plain pointers; torch is only used by callers for device
memory and streams.  There is no CPU fallback: if the library or a GPU is
missing, calls raise ``NipError``.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from . import build as _build

__all__ = ["NipError", "Model", "parse_model", "lib", "forward_backward_inference",
           "forward_backward_inference_host", "forward_inference", "forward_inference_host",
           "most_likely_states", "most_likely_states_host", "Stream",
           "forward_backward_inference_soft", "forward_inference_soft",
           "forward_backward_inference_soft_host", "forward_inference_soft_host",
           "most_likely_states_soft", "most_likely_states_soft_host",
           "e_step", "estep_partial", "estep_finalize", "em_learn", "read_timeseries",
           "e_step_soft", "estep_partial_soft", "e_step_soft_host", "em_learn_soft",
           "write_uncertainseries", "write_model", "em_learn_series", "LIB_PATH"]

LIB_PATH = os.environ.get("NIPAMD_LIB", _build.LIB)

NIP_NO_ERROR = 0
NIP_ERROR_NULLPOINTER = 1
NIP_ERROR_DIVBYZERO = 2
NIP_ERROR_INVALID_ARGUMENT = 3
NIP_ERROR_OUTOFMEMORY = 4
NIP_ERROR_IO = 5
NIP_ERROR_GENERAL = 6
NIP_ERROR_FILENOTFOUND = 7
NIP_ERROR_BAD_LUCK = 8
NIPAMD_ERROR_UNSUPPORTED = 100
NIPAMD_ERROR_DEVICE = 101
STATUS_ZERO_MASS = 1
STATUS_BAD_LUCK = 2
STATUS_BAD_EVIDENCE = 4  # NIPAMD_STATUS_BAD_EVIDENCE: a soft-evidence weight negative, NaN or infinite
ENGINE_AUTO = 0          # interface-chain kernels where they apply, else the general engine
ENGINE_CHAIN = 1         # interface-chain kernels only
ENGINE_JTREE = 2         # the general join-tree engine for every request
STREAM_MAX_LAG = 64      # NIPAMD_STREAM_MAX_LAG
STREAM_CHUNK = 64        # NIPAMD_STREAM_CHUNK: steps per kernel launch of a push

# every entry point declared in include/nip_amd.h
EXPORTS = [
    "nipamd_model_from_spec", "nipamd_model_from_net", "nipamd_model_free",
    "nipamd_model_num_vars", "nipamd_model_var_index", "nipamd_model_var_card",
    "nipamd_model_desc_json", "nipamd_model_param_size", "nipamd_model_gpu_supported",
    "nipamd_fb", "nipamd_fb_host", "nipamd_estep", "nipamd_m_step",
    "nipamd_model_original", "nipamd_model_prior", "nipamd_last_error", "nipamd_last_kernel",
    "nipamd_graph_cliques", "nipamd_estep_partial_size", "nipamd_estep_partial_size_req", "nipamd_estep_partial",
    "nipamd_estep_partial_ex",
    "nipamd_estep_finalize", "nipamd_estep_prefix_first_bad", "nipamd_tree_sum", "nipamd_estep_tail", "nipamd_estep_host", "nipamd_filter", "nipamd_filter_host",
    "nipamd_model_state_name", "nipamd_read_timeseries", "nipamd_series_count",
    "nipamd_series_num_observed", "nipamd_series_observed", "nipamd_series_length",
    "nipamd_series_data", "nipamd_series_free", "nipamd_write_uncertainseries",
    "nipamd_em_learn", "nipamd_write_model", "nipamd_model_var_symbol",
    "nipamd_model_var_label", "nipamd_model_var_info",
    "nipamd_generate_order", "nipamd_generate", "nipamd_generate_host", "nipamd_rand_windows",
    "nipamd_generate_host_draws", "nipamd_likelihood", "nipamd_likelihood_host",
    "nipamd_model_set_engine", "nipamd_jt_plan_dump", "nipamd_hugin_passes",
    "nipamd_model_num_cliques", "nipamd_model_num_sepsets", "nipamd_model_clique",
    "nipamd_model_sepset", "nipamd_model_interface_cliques", "nipamd_model_set_tables", "nipamd_model_fold",
    "nipamd_mlss", "nipamd_mlss_host",
    "nipamd_stream_open", "nipamd_stream_push", "nipamd_stream_flush", "nipamd_stream_reset",
    "nipamd_stream_pending", "nipamd_stream_steps", "nipamd_stream_free",
    "nipamd_stream_push_host", "nipamd_stream_flush_host",
    "nipamd_fb_soft", "nipamd_filter_soft", "nipamd_fb_soft_host", "nipamd_filter_soft_host",
    "nipamd_stream_open_soft", "nipamd_stream_push_soft", "nipamd_stream_push_soft_host",
    "nipamd_mlss_soft", "nipamd_mlss_soft_host",
    "nipamd_estep_soft_partial", "nipamd_estep_soft", "nipamd_estep_soft_host",
]


class NipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("nip_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the gfx950 C-ABI library (raises if it was never built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NipError(NIPAMD_ERROR_DEVICE,
                           "native library missing: %s (run __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.nipamd_model_from_spec.argtypes = [C.c_int, C.POINTER(C.c_char_p), ip, ip, C.c_int,
                                             ip, ip, ip, ip, dp, C.POINTER(vp)]
        L.nipamd_model_from_net.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.nipamd_model_free.argtypes = [vp]
        L.nipamd_model_free.restype = None
        L.nipamd_model_num_vars.argtypes = [vp]
        L.nipamd_model_var_index.argtypes = [vp, C.c_char_p]
        L.nipamd_model_var_card.argtypes = [vp, C.c_int]
        L.nipamd_model_desc_json.argtypes = [vp, C.c_char_p, C.c_int]
        L.nipamd_model_param_size.argtypes = [vp]
        L.nipamd_model_gpu_supported.argtypes = [vp, C.c_int, ip, C.c_int, ip]
        L.nipamd_fb.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip,
                                vp, vp, vp, vp]
        L.nipamd_fb_host.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip,
                                     vp, vp, vp]
        L.nipamd_filter.argtypes = L.nipamd_fb.argtypes
        L.nipamd_filter_host.argtypes = L.nipamd_fb_host.argtypes
        L.nipamd_mlss.argtypes = L.nipamd_fb.argtypes
        L.nipamd_mlss_host.argtypes = L.nipamd_fb_host.argtypes
        L.nipamd_fb_soft.argtypes = [vp, vp, C.c_int, ip, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip,
                                     vp, vp, vp, vp]
        L.nipamd_filter_soft.argtypes = L.nipamd_fb_soft.argtypes
        L.nipamd_fb_soft_host.argtypes = L.nipamd_fb_soft.argtypes[:-1]
        L.nipamd_filter_soft_host.argtypes = L.nipamd_fb_soft_host.argtypes
        L.nipamd_mlss_soft.argtypes = L.nipamd_fb_soft.argtypes
        L.nipamd_mlss_soft_host.argtypes = L.nipamd_fb_soft_host.argtypes
        L.nipamd_estep_soft_partial.argtypes = [vp, vp, C.c_int, ip, vp, C.c_int, ip, C.c_int, C.c_int,
                                                vp, vp, vp, vp]
        L.nipamd_estep_soft.argtypes = L.nipamd_estep_soft_partial.argtypes
        L.nipamd_estep_soft_host.argtypes = L.nipamd_estep_soft_partial.argtypes[:-1]
        L.nipamd_stream_open.argtypes = [vp, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, C.POINTER(vp)]
        L.nipamd_stream_push.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
        L.nipamd_stream_flush.argtypes = [vp, vp, vp, vp, vp]
        L.nipamd_stream_reset.argtypes = [vp, vp]
        L.nipamd_stream_pending.argtypes = [vp]
        L.nipamd_stream_steps.argtypes = [vp]
        L.nipamd_stream_steps.restype = C.c_long
        L.nipamd_stream_free.argtypes = [vp]
        L.nipamd_stream_free.restype = None
        L.nipamd_stream_push_host.argtypes = [vp, vp, C.c_int, vp, vp, vp]
        L.nipamd_stream_flush_host.argtypes = [vp, vp, vp, vp]
        L.nipamd_stream_open_soft.argtypes = [vp, C.c_int, ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int,
                                              C.POINTER(vp)]
        L.nipamd_stream_push_soft.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.nipamd_stream_push_soft_host.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
        L.nipamd_estep.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, vp, vp, vp, vp]
        L.nipamd_estep_partial_size.argtypes = [vp]
        if hasattr(L, "nipamd_estep_partial_size_req"):      # (absent from A/B builds of older revisions)
            L.nipamd_estep_partial_size_req.argtypes = [vp, C.c_int, ip, C.c_int]
        L.nipamd_estep_partial.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, vp, vp, vp, vp]
        if hasattr(L, "nipamd_estep_partial_ex"):            # (absent from A/B builds of older revisions)
            L.nipamd_estep_partial_ex.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, vp, C.c_long, vp, vp, vp]
        L.nipamd_estep_finalize.argtypes = [vp, vp, vp, vp]
        L.nipamd_estep_prefix_first_bad.argtypes = [vp, C.c_int]
        L.nipamd_tree_sum.argtypes = [vp, C.c_long, C.c_int, vp, vp, vp]
        if hasattr(L, "nipamd_estep_tail"):                  # (absent from A/B builds of older revisions)
            L.nipamd_estep_tail.argtypes = [vp, vp, C.c_long, vp, vp, vp]
        L.nipamd_estep_host.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_int, vp, vp, vp]
        L.nipamd_m_step.argtypes = [vp, dp]
        L.nipamd_model_original.argtypes = [vp, C.c_int, dp, C.c_int]
        L.nipamd_model_prior.argtypes = [vp, C.c_int, dp]
        L.nipamd_last_error.restype = C.c_char_p
        L.nipamd_last_kernel.restype = C.c_char_p
        L.nipamd_graph_cliques.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, ip, ip, C.c_int]
        L.nipamd_model_state_name.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.nipamd_read_timeseries.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.nipamd_series_count.argtypes = [vp]
        L.nipamd_series_num_observed.argtypes = [vp]
        L.nipamd_series_observed.argtypes = [vp, ip]
        L.nipamd_series_length.argtypes = [vp, C.c_int]
        L.nipamd_series_data.argtypes = [vp, C.c_int]
        L.nipamd_series_data.restype = C.POINTER(C.c_int32)
        L.nipamd_series_free.argtypes = [vp]
        L.nipamd_series_free.restype = None
        L.nipamd_write_uncertainseries.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, ip, dp, C.c_int,
                                                   C.c_int]
        L.nipamd_em_learn.argtypes = [vp, C.c_int, ip, vp, C.c_int, ip, C.c_double, dp, C.c_int, dp,
                                      C.c_int, ip]
        L.nipamd_write_model.argtypes = [vp, C.c_char_p]
        L.nipamd_model_var_symbol.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise NipError(rc, lib().nipamd_last_error().decode())


def last_kernel() -> str:
    """The dominant kernel of the library's last hot-path launch (a label for
    measurements, nipamd_last_kernel)."""
    return lib().nipamd_last_kernel().decode()


def _ints(xs):
    a = (C.c_int * max(len(xs), 1))()
    for i, x in enumerate(xs):
        a[i] = int(x)
    return a


class Model:
    """A compiled DBN time slice (the reference's nip_model, src/nip.h:71-104)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self._desc = None

    def __del__(self):
        try:
            if self._h:
                lib().nipamd_model_free(self._h)
        except Exception:
            pass

    # -- construction ---------------------------------------------------
    @classmethod
    def from_net(cls, path: str) -> "Model":
        h = C.c_void_p()
        _check(lib().nipamd_model_from_net(path.encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_spec(cls, nodes, potentials) -> "Model":
        """nodes: [(symbol, card, next_symbol_or_None)] in declaration order;
        potentials: [(child, [parents in file order], data_or_None)]."""
        syms = [n[0] for n in nodes]
        idx = {s: i for i, s in enumerate(syms)}
        card = [int(n[1]) for n in nodes]
        nxt = [idx[n[2]] if n[2] else -1 for n in nodes]
        child, npar, par, nd, data = [], [], [], [], []
        for ch, ps, d in potentials:
            child.append(idx[ch]); npar.append(len(ps)); par += [idx[p] for p in ps]
            d = [] if d is None else list(np.asarray(d, np.float64).ravel())
            nd.append(len(d)); data += d
        csyms = (C.c_char_p * len(syms))(*[s.encode() for s in syms])
        dbuf = (C.c_double * max(len(data), 1))(*data)
        h = C.c_void_p()
        _check(lib().nipamd_model_from_spec(len(syms), csyms, _ints(card), _ints(nxt), len(child),
                                            _ints(child), _ints(npar), _ints(par), _ints(nd),
                                            dbuf, C.byref(h)))
        return cls(h.value)

    # -- introspection (the index contract) -----------------------------
    def desc(self) -> dict:
        if self._desc is None:
            n = lib().nipamd_model_desc_json(self._h, None, 0)
            buf = C.create_string_buffer(n + 1)
            lib().nipamd_model_desc_json(self._h, buf, n + 1)
            self._desc = json.loads(buf.value.decode())
        return self._desc

    @property
    def num_vars(self):
        return lib().nipamd_model_num_vars(self._h)

    def variable(self, symbol: str) -> int:
        """model_variable() (src/nip.c:1584): index of a symbol, or -1."""
        return lib().nipamd_model_var_index(self._h, symbol.encode())

    def state_names(self, v: int):
        """The variable's state names (nip_variable_state_name)."""
        out = []
        for st in range(self.card(v)):
            n = lib().nipamd_model_state_name(self._h, v, st, None, 0)
            buf = C.create_string_buffer(n + 1)
            lib().nipamd_model_state_name(self._h, v, st, buf, n + 1)
            out.append(buf.value.decode())
        return out

    def card(self, v: int) -> int:
        return lib().nipamd_model_var_card(self._h, int(v))

    def param_size(self) -> int:
        return lib().nipamd_model_param_size(self._h)

    def gpu_supported(self, obs_vars, query) -> bool:
        return bool(lib().nipamd_model_gpu_supported(self._h, len(obs_vars), _ints(obs_vars),
                                                     len(query), _ints(query)))

    def partial_size(self, obs_vars=None, T: int = 0) -> int:
        """Doubles in an e_step partial: the count body plus the 3-slot route
        tag (nipamd_estep_partial_size), and for a request (obs_vars, T) that
        runs the operator chain's e_step its section as well
        (nipamd_estep_partial_size_req); -1 without an e_step plan."""
        if obs_vars is None:
            return lib().nipamd_estep_partial_size(self._h)
        return lib().nipamd_estep_partial_size_req(self._h, len(obs_vars), _ints(obs_vars), int(T))

    def estep_prefix_first_bad(self, T: int) -> int:
        """nipamd_estep_prefix_first_bad: the first step k < T at which the
        reference's e_step rejects a series that observed nothing at steps
        0..k (-1: none; -2: model too large to simulate).  Host only."""
        return lib().nipamd_estep_prefix_first_bad(self._h, int(T))

    def estep_supported(self) -> bool:
        """Whether the batched e_step has a GPU plan for this model under the
        selected engine (the chain kernel's HMM slice, or the general engine)."""
        return lib().nipamd_estep_partial_size(self._h) >= 0

    def set_engine(self, engine: int) -> int:
        """nipamd_model_set_engine: ENGINE_AUTO / ENGINE_CHAIN / ENGINE_JTREE;
        returns the previous setting."""
        L = lib()
        L.nipamd_model_set_engine.argtypes = [C.c_void_p, C.c_int]
        prev = L.nipamd_model_set_engine(self._h, int(engine))
        if prev < 0:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "bad engine %r" % engine)
        return prev

    def fold(self, keep: int = -1, cards: int = 0):
        """nipamd_model_fold: the interface chain's transition summed over the
        in-clique's hidden parents on the GPU ([64][64], row = previous state),
        or hidden parent `keep`'s table ([card][64][64], `cards` = its card).
        Returns (table, kernel_ms, bytes streamed)."""
        n = (cards if keep >= 0 else 1) * 64 * 64
        out = np.zeros(n)
        ms, by = C.c_double(0.0), C.c_double(0.0)
        L = lib()
        L.nipamd_model_fold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
        _check(L.nipamd_model_fold(self._h, int(keep), out.ctypes.data_as(C.c_void_p), n,
                                   C.byref(ms), C.byref(by)))
        return (out.reshape(64, 64) if keep < 0 else out.reshape(cards, 64, 64)), ms.value, by.value

    def original(self, c: int) -> np.ndarray:
        n = lib().nipamd_model_original(self._h, c, None, 0)
        out = np.zeros(n)
        lib().nipamd_model_original(self._h, c, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    def prior(self, v: int):
        out = np.zeros(self.card(v))
        n = lib().nipamd_model_prior(self._h, v, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out if n > 0 else None

    def m_step(self, params) -> None:
        """m_step() (src/nip.c:2010): params in the em_learn layout."""
        p = np.ascontiguousarray(params, np.float64)
        assert p.size == self.param_size()
        _check(lib().nipamd_m_step(self._h, p.ctypes.data_as(C.POINTER(C.c_double))))
        self._desc = None


def graph_cliques(card, edges, set_parents=True):
    """Clique array of a DAG through the join-tree compiler (index contract)."""
    n = len(card)
    flat = [x for e in edges for x in e]
    off = (C.c_int * (n + 1))()
    cap = n * n
    out = (C.c_int * cap)()
    nc = lib().nipamd_graph_cliques(n, _ints(card), len(edges), _ints(flat), int(set_parents),
                                    off, out, cap)
    if nc < 0:
        raise NipError(-nc, lib().nipamd_last_error().decode())
    return [[out[j] for j in range(off[i], off[i + 1])] for i in range(nc)]


def parse_model(path: str) -> Model:
    """parse_model() (src/nip.c:122): read a Hugin .net file."""
    return Model.from_net(path)


def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


def _out_buf(t, shape, dtype, dev, name):
    """A caller-supplied output buffer must be exactly what the kernels write
    through its raw pointer: shape, dtype, device and dense layout; None
    allocates one."""
    import torch
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if (tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev
            or not t.is_contiguous()):
        raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                       "%s must be a contiguous %s tensor of shape %s on %s (got %s %s on %s)"
                       % (name, dtype, tuple(shape), dev, t.dtype, tuple(t.shape), t.device))
    return t


def _run_device(fn, model, obs, obs_vars, query, post, ll, status, stream):
    import torch
    if obs.dim() == 2:
        obs = obs.unsqueeze(-1)
    assert obs.dtype == torch.int32 and obs.is_cuda and obs.is_contiguous()
    B, T, nobs = obs.shape
    assert nobs == len(obs_vars)
    width = sum(model.card(v) for v in query)
    dev = obs.device
    post = _out_buf(post, (B, T, width), torch.float64, dev, "post")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _check(fn(model._h, C.c_void_p(obs.data_ptr()), nobs, _ints(obs_vars), B, T,
              len(query), _ints(query), C.c_void_p(post.data_ptr()),
              C.c_void_p(ll.data_ptr()), C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    return post, ll, status


def _run_host(fn, model, obs, obs_vars, query):
    obs = np.ascontiguousarray(np.asarray(obs, np.int32))
    if obs.ndim == 2:
        obs = obs[:, :, None]
    B, T, nobs = obs.shape
    width = sum(model.card(v) for v in query)
    post = np.zeros((B, T, width))
    ll = np.zeros(B)
    status = np.zeros(B, np.uint32)
    _check(fn(model._h, obs.ctypes.data_as(C.c_void_p), nobs, _ints(obs_vars),
              B, T, len(query), _ints(query), post.ctypes.data_as(C.c_void_p),
              ll.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
    return post, ll, status


def forward_backward_inference(model: Model, obs, obs_vars, query, post=None, ll=None,
                               status=None, stream=None):
    """Batched forward_backward_inference() (src/nip.c:1320) on the GPU.

    obs: torch int32 CUDA tensor [B, T, n_obs] (state index, <0 missing).
    Returns (post [B, T, sum card(query)] float64, ll [B] float64, status [B] int32),
    all CUDA tensors, computed asynchronously on ``stream`` (default: torch's
    current stream).  ll is the SUM over t, as the reference returns it.
    """
    return _run_device(lib().nipamd_fb, model, obs, obs_vars, query, post, ll, status, stream)


def forward_inference(model: Model, obs, obs_vars, query, post=None, ll=None, status=None,
                      stream=None):
    """Batched forward_inference() (src/nip.c:1103-1315) on the GPU: filtered
    marginals P(X_t | y_0..y_t) of the query variables, and the same ll (sum
    over t).  Buffers and conventions as forward_backward_inference."""
    return _run_device(lib().nipamd_filter, model, obs, obs_vars, query, post, ll, status, stream)


def forward_backward_inference_host(model: Model, obs, obs_vars, query):
    """Same, from host numpy buffers (PCIe-inclusive, synchronous)."""
    return _run_host(lib().nipamd_fb_host, model, obs, obs_vars, query)


def forward_inference_host(model: Model, obs, obs_vars, query):
    """forward_inference from host numpy buffers (PCIe-inclusive, synchronous)."""
    return _run_host(lib().nipamd_filter_host, model, obs, obs_vars, query)


def _soft_device_inputs(model, obs, obs_vars, lik, soft_vars):
    """The device inputs of a soft-evidence call, checked: obs (None when
    obs_vars is empty and lik is given) and lik (None when soft_vars is empty)
    must be exactly what the kernel reads through their raw pointers; B and T
    come from whichever is given.  Returns (obs, B, T, device)."""
    import torch
    W = sum(model.card(v) for v in soft_vars)
    shape = None
    if lik is not None or len(soft_vars):
        if (not torch.is_tensor(lik) or lik.dtype != torch.float64 or not lik.is_cuda or not lik.is_contiguous()
                or lik.dim() != 3 or lik.shape[2] != W):
            got = " (got %s %s on %s)" % (lik.dtype, tuple(lik.shape), lik.device) if torch.is_tensor(lik) else ""
            raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                           "lik must be a contiguous float64 CUDA tensor of shape (B, T, %d)%s" % (W, got))
        shape, dev = (int(lik.shape[0]), int(lik.shape[1])), lik.device
    if obs is None:
        if len(obs_vars) or shape is None:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs may be None only when obs_vars is empty and lik is given")
    else:
        if torch.is_tensor(obs) and obs.dim() == 2:
            obs = obs.unsqueeze(-1)
        if (not torch.is_tensor(obs) or obs.dtype != torch.int32 or not obs.is_cuda or not obs.is_contiguous()
                or obs.dim() != 3 or obs.shape[2] != len(obs_vars)
                or (shape is not None and (tuple(obs.shape[:2]) != shape or obs.device != dev))):
            raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                           "obs must be a contiguous int32 CUDA tensor of shape (B, T, %d), B and T and the device "
                           "as lik's" % len(obs_vars))
        shape, dev = (int(obs.shape[0]), int(obs.shape[1])), obs.device
    return obs, shape[0], shape[1], dev


def _soft_host_inputs(model, obs, obs_vars, lik, soft_vars):
    """The host inputs of a soft-evidence call as contiguous arrays, checked.
    Returns (obs, lik, B, T)."""
    W = sum(model.card(v) for v in soft_vars)
    B = T = None
    if lik is not None:
        lik = np.ascontiguousarray(np.asarray(lik, np.float64))
        if lik.ndim != 3 or lik.shape[2] != W:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "lik must have shape (B, T, %d) (got %s)" % (W, lik.shape))
        B, T = lik.shape[:2]
    elif len(soft_vars):
        raise NipError(NIP_ERROR_INVALID_ARGUMENT, "lik must have shape (B, T, %d)" % W)
    if obs is not None:
        obs = np.ascontiguousarray(np.asarray(obs, np.int32))
        if obs.ndim == 2:
            obs = obs[:, :, None]
        if obs.ndim != 3 or obs.shape[2] != len(obs_vars) or (B is not None and obs.shape[:2] != (B, T)):
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs must have shape (%s, %s, %d) (got %s)"
                           % ("B" if B is None else B, "T" if T is None else T, len(obs_vars), obs.shape))
        B, T = obs.shape[:2]
    elif len(obs_vars) or B is None:
        raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs may be None only when obs_vars is empty and lik is given")
    return obs, lik, B, T


def _soft_call(fn, model, obs, obs_vars, lik, soft_vars, query, B, T, out, ll, status, *stream):
    """fn over checked inputs and outputs: torch tensors on the device (then
    with the stream), numpy arrays on the host."""
    ptr = (lambda a: C.c_void_p(a.data_ptr())) if stream else (lambda a: a.ctypes.data_as(C.c_void_p))
    _check(fn(model._h, ptr(obs) if obs is not None and len(obs_vars) else None, len(obs_vars), _ints(obs_vars),
              ptr(lik) if lik is not None and len(soft_vars) else None, len(soft_vars), _ints(soft_vars), B, T,
              len(query), _ints(query), ptr(out), ptr(ll), ptr(status), *stream))


def _run_soft_device(fn, model, obs, obs_vars, lik, soft_vars, query, post, ll, status, stream):
    import torch
    obs, B, T, dev = _soft_device_inputs(model, obs, obs_vars, lik, soft_vars)
    width = sum(model.card(v) for v in query)
    post = _out_buf(post, (B, T, width), torch.float64, dev, "post")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _soft_call(fn, model, obs, obs_vars, lik, soft_vars, query, B, T, post, ll, status, _stream_ptr(stream))
    return post, ll, status


def _run_soft_host(fn, model, obs, obs_vars, lik, soft_vars, query):
    obs, lik, B, T = _soft_host_inputs(model, obs, obs_vars, lik, soft_vars)
    width = sum(model.card(v) for v in query)
    post = np.zeros((B, T, width))
    ll = np.zeros(B)
    status = np.zeros(B, np.uint32)
    _soft_call(fn, model, obs, obs_vars, lik, soft_vars, query, B, T, post, ll, status)
    return post, ll, status


def forward_backward_inference_soft(model: Model, obs, obs_vars, lik, soft_vars, query, post=None, ll=None,
                                    status=None, stream=None):
    """Batched smoothing under hard and soft (likelihood) evidence on the GPU
    (nipamd_fb_soft; the reference's insert_soft_evidence, src/nip.c:967-1030).

    obs: torch int32 CUDA tensor [B, T, len(obs_vars)] (state index, <0
    missing), or None when obs_vars is empty.  lik: contiguous float64 CUDA
    tensor [B, T, W], W = sum card(soft_vars): each step's likelihood vectors
    in soft_vars order -- the row layout of ``post`` for query = soft_vars, so
    the rows of forward_backward_inference can be fed back in; None when
    soft_vars is empty.  Weights are non-negative and finite, not necessarily
    normalised (all ones: not observed; one-hot: a hard observation); a
    negative, NaN or infinite weight leaves its sequence without mass from that
    step on, with STATUS_BAD_EVIDENCE | STATUS_ZERO_MASS.  query: the model's
    interface variable, or members of a joint interface (any subset, any order).
    Returns (post [B, T, sum card(query)], ll [B], status [B]), CUDA tensors,
    computed asynchronously on ``stream`` (default: torch's current stream)."""
    return _run_soft_device(lib().nipamd_fb_soft, model, obs, obs_vars, lik, soft_vars, query, post, ll, status,
                            stream)


def forward_inference_soft(model: Model, obs, obs_vars, lik, soft_vars, query, post=None, ll=None, status=None,
                           stream=None):
    """Batched filtering under hard and soft evidence (nipamd_filter_soft):
    P(X_t | evidence of steps 0..t) and the same ll.  Buffers and conventions
    as forward_backward_inference_soft."""
    return _run_soft_device(lib().nipamd_filter_soft, model, obs, obs_vars, lik, soft_vars, query, post, ll, status,
                            stream)


def forward_backward_inference_soft_host(model: Model, obs, obs_vars, lik, soft_vars, query):
    """forward_backward_inference_soft from host numpy buffers (PCIe-inclusive, synchronous)."""
    return _run_soft_host(lib().nipamd_fb_soft_host, model, obs, obs_vars, lik, soft_vars, query)


def forward_inference_soft_host(model: Model, obs, obs_vars, lik, soft_vars, query):
    """forward_inference_soft from host numpy buffers (PCIe-inclusive, synchronous)."""
    return _run_soft_host(lib().nipamd_filter_soft_host, model, obs, obs_vars, lik, soft_vars, query)


def most_likely_states(model: Model, obs, obs_vars, query, path=None, logp=None, status=None,
                       stream=None):
    """Batched mlss() (declared in src/nip.h:431-438, never implemented in the
    reference): the most likely sequence of the interface given the evidence
    (Viterbi), on the GPU.

    obs: torch int32 CUDA tensor [B, T, n_obs] (state index, <0 missing);
    query: the model's interface variable(s), all of them.  Returns
    (path [B, T, len(query)] int32, logp [B] float64, status [B] int32), CUDA
    tensors, computed asynchronously on ``stream`` (default: torch's current
    stream).  A sequence without mass has status STATUS_ZERO_MASS, logp
    -DBL_MAX and a path of -1.
    """
    import torch
    if obs.dim() == 2:
        obs = obs.unsqueeze(-1)
    assert obs.dtype == torch.int32 and obs.is_cuda and obs.is_contiguous()
    B, T, nobs = obs.shape
    assert nobs == len(obs_vars)
    dev = obs.device
    path = _out_buf(path, (B, T, len(query)), torch.int32, dev, "path")
    logp = _out_buf(logp, (B,), torch.float64, dev, "logp")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _check(lib().nipamd_mlss(model._h, C.c_void_p(obs.data_ptr()), nobs, _ints(obs_vars), B, T,
                             len(query), _ints(query), C.c_void_p(path.data_ptr()),
                             C.c_void_p(logp.data_ptr()), C.c_void_p(status.data_ptr()),
                             _stream_ptr(stream)))
    return path, logp, status


def most_likely_states_host(model: Model, obs, obs_vars, query):
    """most_likely_states from host numpy buffers (PCIe-inclusive, synchronous)."""
    obs = np.ascontiguousarray(np.asarray(obs, np.int32))
    if obs.ndim == 2:
        obs = obs[:, :, None]
    B, T, nobs = obs.shape
    path = np.zeros((B, T, len(query)), np.int32)
    logp = np.zeros(B)
    status = np.zeros(B, np.uint32)
    _check(lib().nipamd_mlss_host(model._h, obs.ctypes.data_as(C.c_void_p), nobs, _ints(obs_vars),
                                  B, T, len(query), _ints(query), path.ctypes.data_as(C.c_void_p),
                                  logp.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
    return path, logp, status


def most_likely_states_soft(model: Model, obs, obs_vars, lik, soft_vars, query, path=None, logp=None, status=None,
                            stream=None):
    """most_likely_states under hard and soft (likelihood) evidence on the GPU
    (nipamd_mlss_soft): the most likely sequence of the interface with every
    child summed out, a soft child under its likelihood vector -- so the
    posterior rows of one model decode the next without being cut down to
    their arg-max.

    obs, obs_vars, lik, soft_vars: as forward_backward_inference_soft takes
    them (lik float64 [B, T, sum card(soft_vars)], obs None when obs_vars is
    empty).  query: the model's interface variable(s), all of them.  Returns
    (path [B, T, len(query)] int32, logp [B] float64, status [B] int32), CUDA
    tensors, computed asynchronously on ``stream``.  logp is that of the
    weights as given: scaling a step's vector by 2^k adds k ln 2 and moves no
    path.  A sequence without mass has STATUS_ZERO_MASS (with
    STATUS_BAD_EVIDENCE after a negative, NaN or infinite weight), logp
    -DBL_MAX and a path of -1."""
    import torch
    obs, B, T, dev = _soft_device_inputs(model, obs, obs_vars, lik, soft_vars)
    path = _out_buf(path, (B, T, len(query)), torch.int32, dev, "path")
    logp = _out_buf(logp, (B,), torch.float64, dev, "logp")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _soft_call(lib().nipamd_mlss_soft, model, obs, obs_vars, lik, soft_vars, query, B, T, path, logp, status,
               _stream_ptr(stream))
    return path, logp, status


def most_likely_states_soft_host(model: Model, obs, obs_vars, lik, soft_vars, query):
    """most_likely_states_soft from host numpy buffers (PCIe-inclusive, synchronous)."""
    obs, lik, B, T = _soft_host_inputs(model, obs, obs_vars, lik, soft_vars)
    path = np.zeros((B, T, len(query)), np.int32)
    logp = np.zeros(B)
    status = np.zeros(B, np.uint32)
    _soft_call(lib().nipamd_mlss_soft_host, model, obs, obs_vars, lik, soft_vars, query, B, T, path, logp, status)
    return path, logp, status


class Stream:
    """Online inference over B sequences that advance in lockstep: resumable
    filtering (lag = 0) and fixed-lag smoothing (nipamd_stream_*).

    Row t is the marginal of the query variables at step t given the evidence
    of steps 0 .. t + lag (at a flush: up to the last step consumed).  A push
    of T steps returns the E = max(0, pending + T - lag) rows whose lag it
    consumed, [B, E, sum card(query)]; flush() returns the `pending` rows
    left.  ``ll`` and ``status`` hold the running totals after the last call
    (CUDA tensors [B], written asynchronously on the call's stream).  Rows, ll
    and status do not depend on how the steps are split into pushes.

    query: the model's interface variable, or members of a joint interface (any
    subset, any order).  The stream keeps its Model alive; close() (or the
    context manager) frees the device state.

    soft_vars: variables whose evidence arrives as likelihood vectors
    (nipamd_stream_open_soft / nipamd_stream_push_soft): every push then takes
    ``lik``, float64 [B, T, W] with W = sum card(soft_vars), a step's vectors in
    soft_vars order -- the weights of forward_backward_inference_soft, and the
    row layout of another stream's rows for query = soft_vars.  ``obs`` may be
    None when obs_vars is empty.  A weight that is negative, NaN or infinite
    sets STATUS_BAD_EVIDENCE | STATUS_ZERO_MASS from its step on.
    """

    def __init__(self, model: Model, obs_vars, query, B: int, lag: int = 0, soft_vars=()):
        self._h = None
        self.model = model
        self.obs_vars = [int(v) for v in obs_vars]
        self.soft_vars = [int(v) for v in soft_vars]
        self.query = [int(v) for v in query]
        self.B, self.lag = int(B), int(lag)
        h = C.c_void_p()
        if self.soft_vars:
            _check(lib().nipamd_stream_open_soft(model._h, len(self.obs_vars), _ints(self.obs_vars),
                                                 len(self.soft_vars), _ints(self.soft_vars), len(self.query),
                                                 _ints(self.query), self.B, self.lag, C.byref(h)))
        else:
            _check(lib().nipamd_stream_open(model._h, len(self.obs_vars), _ints(self.obs_vars), len(self.query),
                                            _ints(self.query), self.B, self.lag, C.byref(h)))
        self._h = h
        self.width = sum(model.card(v) for v in self.query)
        self.lik_width = sum(model.card(v) for v in self.soft_vars)
        import torch
        self.ll = torch.zeros((self.B,), dtype=torch.float64, device="cuda")
        self.status = torch.zeros((self.B,), dtype=torch.int32, device="cuda")

    def _handle(self):
        if not self._h:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "the stream is closed")
        return self._h

    @property
    def steps(self) -> int:
        """Steps consumed so far."""
        return lib().nipamd_stream_steps(self._handle())

    @property
    def pending(self) -> int:
        """Rows still owed: min(steps, lag), 0 after a flush."""
        return lib().nipamd_stream_pending(self._handle())

    def _push_soft(self, obs, lik, post, stream):
        """push on a stream with soft columns: lik checked as
        forward_backward_inference_soft checks it, obs against it."""
        import torch
        h = self._handle()
        W = self.lik_width
        if (not torch.is_tensor(lik) or lik.dtype != torch.float64 or not lik.is_cuda or not lik.is_contiguous()
                or lik.dim() != 3 or lik.shape[0] != self.B or lik.shape[2] != W):
            got = " (got %s %s on %s)" % (lik.dtype, tuple(lik.shape), lik.device) if torch.is_tensor(lik) else ""
            raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                           "lik must be a contiguous float64 CUDA tensor of shape (%d, T, %d)%s" % (self.B, W, got))
        T, dev = int(lik.shape[1]), lik.device
        if obs is None:
            if len(self.obs_vars):
                raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs may be None only when obs_vars is empty")
        else:
            if torch.is_tensor(obs) and obs.dim() == 2:
                obs = obs.unsqueeze(-1)
            if (not torch.is_tensor(obs) or obs.dtype != torch.int32 or not obs.is_cuda or not obs.is_contiguous()
                    or obs.dim() != 3 or obs.shape[2] != len(self.obs_vars)
                    or tuple(obs.shape[:2]) != (self.B, T) or obs.device != dev):
                raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                               "obs must be a contiguous int32 CUDA tensor of shape (%d, %d, %d) on lik's device"
                               % (self.B, T, len(self.obs_vars)))
        E = max(0, self.pending + T - self.lag)
        post = _out_buf(post, (self.B, E, self.width), torch.float64, dev, "post")
        _check(lib().nipamd_stream_push_soft(h, C.c_void_p(obs.data_ptr() if len(self.obs_vars) else 0),
                                             C.c_void_p(lik.data_ptr()), T, C.c_void_p(post.data_ptr() if E else 0),
                                             C.c_void_p(self.ll.data_ptr()), C.c_void_p(self.status.data_ptr()),
                                             _stream_ptr(stream)))
        return post

    def push(self, obs, post=None, stream=None, lik=None):
        """obs: torch int32 CUDA tensor [B, T, n_obs] (state index, <0 missing), T >= 1;
        lik: with soft_vars, torch float64 CUDA tensor [B, T, W]."""
        import torch
        h = self._handle()
        if self.soft_vars:
            return self._push_soft(obs, lik, post, stream)
        if lik is not None:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "lik given to a stream without soft_vars")
        if obs.dim() == 2:
            obs = obs.unsqueeze(-1)
        if (obs.dtype != torch.int32 or not obs.is_cuda or not obs.is_contiguous() or obs.dim() != 3
                or obs.shape[0] != self.B or obs.shape[2] != len(self.obs_vars)):
            raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                           "obs must be a contiguous int32 CUDA tensor of shape (%d, T, %d)"
                           % (self.B, len(self.obs_vars)))
        T = int(obs.shape[1])
        E = max(0, self.pending + T - self.lag)
        post = _out_buf(post, (self.B, E, self.width), torch.float64, obs.device, "post")
        _check(lib().nipamd_stream_push(h, C.c_void_p(obs.data_ptr()), T,
                                        C.c_void_p(post.data_ptr() if E else 0),
                                        C.c_void_p(self.ll.data_ptr()), C.c_void_p(self.status.data_ptr()),
                                        _stream_ptr(stream)))
        return post

    def flush(self, post=None, stream=None):
        """The rows left, each given every step consumed; then only reset() or close()."""
        import torch
        h = self._handle()
        E = self.pending
        post = _out_buf(post, (self.B, E, self.width), torch.float64, self.ll.device, "post")
        _check(lib().nipamd_stream_flush(h, C.c_void_p(post.data_ptr() if E else 0),
                                         C.c_void_p(self.ll.data_ptr()), C.c_void_p(self.status.data_ptr()),
                                         _stream_ptr(stream)))
        return post

    def _push_soft_host(self, obs, lik):
        h = self._handle()
        W = self.lik_width
        if lik is None:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "lik must have shape (%d, T, %d)" % (self.B, W))
        lik = np.ascontiguousarray(np.asarray(lik, np.float64))
        if lik.ndim != 3 or lik.shape[0] != self.B or lik.shape[2] != W:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT,
                           "lik must have shape (%d, T, %d) (got %s)" % (self.B, W, lik.shape))
        T = int(lik.shape[1])
        if obs is not None:
            obs = np.ascontiguousarray(np.asarray(obs, np.int32))
            if obs.ndim == 2:
                obs = obs[:, :, None]
            if obs.shape != (self.B, T, len(self.obs_vars)):
                raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs must have shape (%d, %d, %d) (got %s)"
                               % (self.B, T, len(self.obs_vars), obs.shape))
        elif len(self.obs_vars):
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs may be None only when obs_vars is empty")
        post = np.zeros((self.B, max(0, self.pending + T - self.lag), self.width))
        ll, status = np.zeros(self.B), np.zeros(self.B, np.uint32)
        _check(lib().nipamd_stream_push_soft_host(
            h, obs.ctypes.data_as(C.c_void_p) if obs is not None and len(self.obs_vars) else None,
            lik.ctypes.data_as(C.c_void_p), T, post.ctypes.data_as(C.c_void_p), ll.ctypes.data_as(C.c_void_p),
            status.ctypes.data_as(C.c_void_p)))
        return post, ll, status

    def push_host(self, obs, lik=None):
        """push from host numpy arrays, obs [B, T, n_obs] and with soft_vars lik
        [B, T, W]: (post, ll, status) as numpy (synchronous)."""
        h = self._handle()
        if self.soft_vars:
            return self._push_soft_host(obs, lik)
        if lik is not None:
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "lik given to a stream without soft_vars")
        obs = np.ascontiguousarray(np.asarray(obs, np.int32))
        if obs.ndim == 2:
            obs = obs[:, :, None]
        if obs.ndim != 3 or obs.shape[0] != self.B or obs.shape[2] != len(self.obs_vars):
            raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs must have shape (%d, T, %d)" % (self.B, len(self.obs_vars)))
        T = int(obs.shape[1])
        post = np.zeros((self.B, max(0, self.pending + T - self.lag), self.width))
        ll, status = np.zeros(self.B), np.zeros(self.B, np.uint32)
        _check(lib().nipamd_stream_push_host(h, obs.ctypes.data_as(C.c_void_p), T, post.ctypes.data_as(C.c_void_p),
                                             ll.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return post, ll, status

    def flush_host(self):
        h = self._handle()
        post = np.zeros((self.B, self.pending, self.width))
        ll, status = np.zeros(self.B), np.zeros(self.B, np.uint32)
        _check(lib().nipamd_stream_flush_host(h, post.ctypes.data_as(C.c_void_p), ll.ctypes.data_as(C.c_void_p),
                                              status.ctypes.data_as(C.c_void_p)))
        return post, ll, status

    def reset(self, stream=None):
        """Back to the prior: no step consumed, ll = 0, status = 0."""
        _check(lib().nipamd_stream_reset(self._handle(), _stream_ptr(stream)))
        self.ll.zero_()
        self.status.zero_()

    def close(self):
        if self._h:
            lib().nipamd_stream_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generate_order(model: Model):
    """The sampling order of generate_data (src/nip.c:2343-2375): the model
    variable of each data column."""
    L = lib()
    n = L.nipamd_generate_order(model._h, None)
    order = (C.c_int * max(n, 1))()
    L.nipamd_generate_order(model._h, order)
    return list(order)[:n]


def generate_data(model: Model, seed: int, B: int, T: int, out=None, stream=None):
    """generate_data (src/nip.c:2325-2478) B times from srand(seed), on the
    GPU: (order, int32 tensor [B][T][nv]); column i holds variable order[i]
    (the reference's ts->observed)."""
    import torch
    order = generate_order(model)
    if out is None:
        out = torch.empty((B, T, len(order)), dtype=torch.int32, device="cuda")
    assert out.dtype == torch.int32 and out.is_cuda and out.is_contiguous()
    assert tuple(out.shape) == (B, T, len(order))
    L = lib()
    L.nipamd_generate.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.nipamd_generate(model._h, seed, B, T, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return order, out


def likelihood(model: Model, obs, obs_vars, marked):
    """util/niplikelihood.c batched on the GPU: (m1, m2, ll) [B][T] -- the
    mass after the unmarked columns' evidence, after all, and log(m2/m1)
    per step, each step on its own (niplikelihood.c:111-133)."""
    obs = np.ascontiguousarray(np.asarray(obs, np.int32))
    if obs.ndim == 2:
        obs = obs[:, :, None]
    B, T, nobs = obs.shape
    if not (len(obs_vars) == nobs == len(marked)):
        raise NipError(NIP_ERROR_INVALID_ARGUMENT, "obs_vars (%d) and marked (%d) must name every "
                       "one of the %d columns" % (len(obs_vars), len(marked), nobs))
    out = [np.zeros((B, T)) for _ in range(3)]
    L = lib()
    L.nipamd_likelihood_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(L.nipamd_likelihood_host(model._h, obs.ctypes.data_as(C.c_void_p), nobs, _ints(obs_vars),
                                    _ints([1 if m else 0 for m in marked]), B, T,
                                    *[o.ctypes.data_as(C.c_void_p) for o in out]))
    return tuple(out)


def rand_windows(seed: int, B: int, draws_per_series: int):
    """glibc rand() state window [B][31] of each series (nipamd_rand_windows)."""
    out = np.zeros((B, 31), np.uint32)
    L = lib()
    L.nipamd_rand_windows.argtypes = [C.c_long, C.c_int, C.c_long, C.c_void_p]
    _check(L.nipamd_rand_windows(seed, B, draws_per_series, out.ctypes.data_as(C.c_void_p)))
    return out


def read_timeseries(model: Model, path):
    """read_timeseries() (src/nip.c:512-667) of the reference's data-file format.

    Returns (series, obs_vars): a list of int32 arrays [T_i, n_obs] (state
    index, -1 missing) and the model variable of each column (file order).
    """
    h = C.c_void_p()
    _check(lib().nipamd_read_timeseries(model._h, os.fsencode(path), C.byref(h)))
    try:
        L = lib()
        n, k = L.nipamd_series_count(h), L.nipamd_series_num_observed(h)
        ov = (C.c_int * max(k, 1))()
        _check(L.nipamd_series_observed(h, ov))
        out = []
        for i in range(n):
            T = L.nipamd_series_length(h, i)
            if k == 0:
                out.append(np.zeros((T, 0), np.int32))
                continue
            p = L.nipamd_series_data(h, i)
            out.append(np.ctypeslib.as_array(p, shape=(T * k,)).reshape(T, k).copy())
        return out, [ov[i] for i in range(k)]
    finally:
        lib().nipamd_series_free(h)


def write_model(model: Model, path):
    """write_model() (src/nip.c:298-484): the model as a Hugin .net file."""
    _check(lib().nipamd_write_model(model._h, os.fsencode(path)))


def em_learn_series(model: Model, series, obs_vars, threshold, init=None, max_iterations=0):
    """em_learn() for series of any lengths on one GPU (nipamd_em_learn).

    series: list of int32 arrays [T_i, n_obs].  init: initial parameters in the
    em_learn layout, or None for rand()/RAND_MAX draws like the reference (C
    rand(); seed it with libc's srand).  Returns (rc, learning_curve)."""
    series = [np.ascontiguousarray(np.asarray(s, np.int32).reshape(len(s), -1)) for s in series]
    k = len(obs_vars)
    flat = np.ascontiguousarray(np.concatenate(series, axis=0)) if k else np.zeros(1, np.int32)
    lengths = np.array([len(s) for s in series], np.int32)
    cap = 100000
    curve = np.zeros(cap)
    n = C.c_int(0)
    ini = None if init is None else np.ascontiguousarray(init, np.float64)
    rc = lib().nipamd_em_learn(model._h, len(series), lengths.ctypes.data_as(C.POINTER(C.c_int)),
                               flat.ctypes.data_as(C.c_void_p), k, _ints(obs_vars), threshold,
                               None if ini is None else ini.ctypes.data_as(C.POINTER(C.c_double)),
                               max_iterations, curve.ctypes.data_as(C.POINTER(C.c_double)), cap,
                               C.byref(n))
    if rc not in (0, 8):
        _check(rc)
    return rc, list(curve[:n.value])


def write_uncertainseries(model: Model, path, var: int, posts):
    """write_uncertainseries() (src/nip.c:815-893): `posts` is a list of
    arrays [T_i, card(var)] (or wider rows with the variable first)."""
    posts = [np.ascontiguousarray(p, np.float64) for p in posts]
    stride = posts[0].shape[1]
    flat = np.ascontiguousarray(np.concatenate(posts, axis=0))
    lengths = np.array([p.shape[0] for p in posts], np.int32)
    _check(lib().nipamd_write_uncertainseries(
        model._h, os.fsencode(path), var, len(posts), lengths.ctypes.data_as(C.POINTER(C.c_int)),
        flat.ctypes.data_as(C.POINTER(C.c_double)), stride, 0))


def _obs3(obs, obs_vars):
    import torch
    if obs.dim() == 2:
        obs = obs.unsqueeze(-1)
    assert obs.dtype == torch.int32 and obs.is_cuda and obs.is_contiguous()
    assert obs.shape[2] == len(obs_vars)
    return obs


def estep_partial(model: Model, obs, obs_vars, partial=None, ll=None, status=None, stream=None):
    """First half of the batched e_step (src/nip.c:1708): the fixed-order tree
    sum of the per-sequence count slabs of obs [B, T, n_obs] (CUDA int32).
    Returns (partial [partial_size] float64, ll [B], status [B]) on the GPU."""
    import torch
    obs = _obs3(obs, obs_vars)
    B, T, nobs = obs.shape
    L = lib()
    S = (L.nipamd_estep_partial_size_req(model._h, nobs, _ints(obs_vars), T)
         if hasattr(L, "nipamd_estep_partial_size_req") else L.nipamd_estep_partial_size(model._h))
    if S < 0:
        raise NipError(NIPAMD_ERROR_UNSUPPORTED, "model has no GPU e_step plan")
    dev = obs.device
    partial = _out_buf(partial, (S,), torch.float64, dev, "partial")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    if hasattr(L, "nipamd_estep_partial_ex"):
        # with the request's capacity: the operator chain may take the request
        _check(L.nipamd_estep_partial_ex(model._h, C.c_void_p(obs.data_ptr()), nobs, _ints(obs_vars), B, T,
                                         C.c_void_p(partial.data_ptr()), int(partial.numel()),
                                         C.c_void_p(ll.data_ptr()), C.c_void_p(status.data_ptr()),
                                         _stream_ptr(stream)))
    else:
        _check(L.nipamd_estep_partial(model._h, C.c_void_p(obs.data_ptr()), nobs, _ints(obs_vars),
                                      B, T, C.c_void_p(partial.data_ptr()), C.c_void_p(ll.data_ptr()),
                                      C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    return partial, ll, status


def tree_sum(rows, out=None, stream=None):
    """Fixed-order binary-tree sum of rows [n, S] (CUDA float64) over dim 0
    (nipamd_tree_sum): pairs (2i, 2i + 1) level by level, the shape of the
    e_step's count tree.  Returns out [S]."""
    import torch
    x = rows.reshape(rows.shape[0], -1) if rows.dim() > 1 else rows.reshape(-1, 1)
    x = x.to(torch.float64).contiguous()
    n, S = int(x.shape[0]), int(x.shape[1])
    out = _out_buf(out, (S,), torch.float64, x.device, "out")
    work = torch.empty((2 * ((n + 63) // 64) * S,), dtype=torch.float64, device=x.device) if n > 64 else None
    _check(lib().nipamd_tree_sum(C.c_void_p(x.data_ptr()), n, S,
                                 C.c_void_p(work.data_ptr() if work is not None else 0),
                                 C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def estep_tail(ll, status, out=None, stream=None):
    """out [2] = [nipamd_tree_sum of ll [B], number of nonzero status words]
    (nipamd_estep_tail): the scalars em_learn exchanges with its counts,
    written on the GPU next to them (em.py).  Returns out."""
    import torch
    B = int(ll.numel())
    out = _out_buf(out, (2,), torch.float64, ll.device, "out")
    if ll.dtype != torch.float64 or not ll.is_contiguous() or status.numel() != B or status.element_size() != 4 \
            or not status.is_contiguous():
        raise NipError(NIP_ERROR_INVALID_ARGUMENT, "ll must be contiguous float64 [B], status contiguous 32-bit [B]")
    work = torch.empty((2 * ((B + 63) // 64) + (B + 4095) // 4096 + 1,), dtype=torch.float64, device=ll.device)
    _check(lib().nipamd_estep_tail(C.c_void_p(ll.data_ptr()), C.c_void_p(status.data_ptr()), B,
                                   C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def estep_finalize(model: Model, partial, counts, stream=None):
    """counts (CUDA float64 [param_size], em_learn layout) += families of partial.
    counts=None starts from the em_learn pseudo-counts (ones, nip.c:2172)."""
    import torch
    if counts is None:
        counts = torch.ones((model.param_size(),), dtype=torch.float64, device=partial.device)
    counts = _out_buf(counts, (model.param_size(),), torch.float64, partial.device, "counts")
    _check(lib().nipamd_estep_finalize(model._h, C.c_void_p(partial.data_ptr()),
                                       C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
    return counts


def e_step(model: Model, obs, obs_vars, counts=None, ll=None, status=None, stream=None):
    """Batched e_step() (src/nip.c:1708-2007) of B sequences on the GPU.

    counts: CUDA float64 [param_size] accumulated into (default: ones, the
    em_learn pseudo-counts of nip.c:2172).  Returns (counts, ll [B], status [B]);
    status bit NIPAMD_STATUS_BAD_LUCK marks the sequences for which the
    reference's e_step returns NIP_ERROR_BAD_LUCK.
    """
    import torch
    obs = _obs3(obs, obs_vars)
    B, T, nobs = obs.shape
    dev = obs.device
    if counts is None:
        counts = torch.ones((model.param_size(),), dtype=torch.float64, device=dev)
    counts = _out_buf(counts, (model.param_size(),), torch.float64, dev, "counts")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _check(lib().nipamd_estep(model._h, C.c_void_p(obs.data_ptr()), nobs, _ints(obs_vars), B, T,
                              C.c_void_p(counts.data_ptr()), C.c_void_p(ll.data_ptr()),
                              C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    return counts, ll, status


def _estep_soft_call(fn, model, obs, obs_vars, lik, soft_vars, B, T, out, ll, status, *stream):
    """_soft_call without a query: fn over checked inputs and outputs."""
    ptr = (lambda a: C.c_void_p(a.data_ptr())) if stream else (lambda a: a.ctypes.data_as(C.c_void_p))
    _check(fn(model._h, ptr(obs) if obs is not None and len(obs_vars) else None, len(obs_vars), _ints(obs_vars),
              ptr(lik) if lik is not None and len(soft_vars) else None, len(soft_vars), _ints(soft_vars), B, T,
              ptr(out), ptr(ll), ptr(status), *stream))


def estep_partial_soft(model: Model, obs, obs_vars, lik, soft_vars, partial=None, ll=None, status=None, stream=None):
    """First half of the batched e_step under soft evidence
    (nipamd_estep_soft_partial): the fixed-order tree sum of the per-sequence
    count slabs.  obs, lik and the accepted weights as
    forward_backward_inference_soft.  Returns (partial [partial_size] float64,
    ll [B], status [B]) on the GPU; the partial is a wide-chain-slab partial,
    which estep_finalize finalises and tree_sum combines with others."""
    import torch
    obs, B, T, dev = _soft_device_inputs(model, obs, obs_vars, lik, soft_vars)
    S = lib().nipamd_estep_partial_size(model._h)
    if S < 0:
        raise NipError(NIPAMD_ERROR_UNSUPPORTED, "model has no GPU e_step plan")
    partial = _out_buf(partial, (S,), torch.float64, dev, "partial")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _estep_soft_call(lib().nipamd_estep_soft_partial, model, obs, obs_vars, lik, soft_vars, B, T, partial, ll, status,
                     _stream_ptr(stream))
    return partial, ll, status


def e_step_soft(model: Model, obs, obs_vars, lik, soft_vars, counts=None, ll=None, status=None, stream=None):
    """Batched e_step under hard and soft (likelihood) evidence on the GPU
    (nipamd_estep_soft): the expected counts of e_step with a soft child's
    count row shared out as the child's posterior given its vector.  All ones
    is the missing observation, a one-hot vector the hard one.  counts: CUDA
    float64 [param_size] accumulated into (default: ones, the em_learn
    pseudo-counts).  Returns (counts, ll [B], status [B]); a sequence without
    mass has STATUS_ZERO_MASS | STATUS_BAD_LUCK and adds nothing to the counts.
    The reference's verdicts on leading missing runs and on ll > 0 do not apply."""
    import torch
    obs, B, T, dev = _soft_device_inputs(model, obs, obs_vars, lik, soft_vars)
    if counts is None:
        counts = torch.ones((model.param_size(),), dtype=torch.float64, device=dev)
    counts = _out_buf(counts, (model.param_size(),), torch.float64, dev, "counts")
    ll = _out_buf(ll, (B,), torch.float64, dev, "ll")
    status = _out_buf(status, (B,), torch.int32, dev, "status")
    _estep_soft_call(lib().nipamd_estep_soft, model, obs, obs_vars, lik, soft_vars, B, T, counts, ll, status,
                     _stream_ptr(stream))
    return counts, ll, status


def e_step_soft_host(model: Model, obs, obs_vars, lik, soft_vars, counts=None):
    """e_step_soft from host numpy buffers (PCIe-inclusive, synchronous).
    counts: float64 [param_size] accumulated into (default: ones)."""
    obs, lik, B, T = _soft_host_inputs(model, obs, obs_vars, lik, soft_vars)
    P = model.param_size()
    if counts is None:
        counts = np.ones(P)
    if not (isinstance(counts, np.ndarray) and counts.dtype == np.float64 and counts.shape == (P,)
            and counts.flags.c_contiguous):
        raise NipError(NIP_ERROR_INVALID_ARGUMENT, "counts must be a contiguous float64 array of shape (%d,)" % P)
    ll = np.zeros(B)
    status = np.zeros(B, np.uint32)
    _estep_soft_call(lib().nipamd_estep_soft_host, model, obs, obs_vars, lik, soft_vars, B, T, counts, ll, status)
    return counts, ll, status


from .em import em_learn  # noqa: E402
from .em_soft import em_learn_soft  # noqa: E402
