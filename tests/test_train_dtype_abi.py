"""The C ABI of the training neuron ops: one entry point per operation with the tensors' dtype as an argument
(include/aura_hip.h, "Surrogate-gradient training path", and aura_lif_run).  An unknown dtype code is refused before
anything is launched; L <= 256 binds the bf16 form alone; no ``_bf16`` twin is left."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, T, H = 2, 1, 8
E_INVAL = -1
L_OPS = ("aura_gif_train_forward", "aura_gif_backward", "aura_gif_prosody_run", "aura_gif_prosody_train_forward",
         "aura_gif_prosody_backward")


def _calls(dev, dtype, L):
    """name -> (the arguments up to the sizes, the tensors the call may write), on valid ROWS x T x H tensors."""
    g = torch.Generator().manual_seed(5)
    mk = lambda t: t.to(dtype).to(dev)
    rnd = lambda *s: mk(torch.randn(*s, generator=g))
    pos = lambda *s: mk(1.0 + 0.3 * torch.rand(*s, generator=g))
    nan = lambda *s, dt=dtype: torch.full(s, float("nan"), dtype=dt, device=dev)
    h, gains, sa, st, ws = rnd(ROWS, T, H), pos(ROWS, T), rnd(ROWS, T, H), pos(ROWS, T, H), rnd(ROWS, T, H)
    x, mem, pre, gs, gm, beta, thr, slope = rnd(ROWS, H), rnd(ROWS, H), rnd(ROWS, H), rnd(ROWS, H), rnd(ROWS, H), \
        pos(H), pos(H), pos(H)
    gif, n3, n2 = (0.9, L, 0.05, 1.0), (ROWS, T, H), (ROWS, H)
    pro = gif + (0.3,)
    calls = {}

    def add(name, make):
        out = dict(a=nan(ROWS, T, H), b=nan(ROWS, T, H), c=nan(ROWS, T, H), v=nan(ROWS, H), th=nan(ROWS, H),
                   f=nan(ROWS, H, dt=torch.float32), gg=nan(ROWS, T, dt=torch.float32))
        calls[name] = (make(out), out)
    add("aura_gif_train_forward", lambda o: (h, o["a"], o["v"], o["th"], o["b"], o["c"], *gif, *n3))
    add("aura_gif_backward", lambda o: (sa, st, ws, o["a"], o["v"], o["th"], *gif, *n3))
    add("aura_lif_run", lambda o: (h, o["a"], o["v"], beta, thr, *n3))
    add("aura_lif_train_forward", lambda o: (x, mem, beta, thr, o["v"], o["th"], o["a"], *n2))
    add("aura_lif_backward", lambda o: (pre, gs, gm, beta, thr, slope, o["v"], o["th"], o["f"], *n2))
    add("aura_gif_prosody_run", lambda o: (h, gains, o["a"], o["v"], o["th"], *pro, *n3))
    add("aura_gif_prosody_train_forward", lambda o: (h, gains, o["a"], o["v"], o["th"], o["b"], o["c"], *pro, *n3))
    add("aura_gif_prosody_backward", lambda o: (sa, st, h, gains, ws, o["a"], o["gg"], o["v"], o["th"], *pro, *n3))
    return calls


def _invoke(name, args, code):
    from aura_snn_rag_amd import _lib
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
    return getattr(_lib.load(), name)(*[ptr(a) for a in args], code, torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("code", [2, -1])
def test_unknown_dtype_code_is_refused_before_any_launch(dev, code):
    """Every entry point, valid fp32 tensors, a dtype code that is neither AURA_DTYPE_F32 nor AURA_DTYPE_BF16:
    AURA_E_INVAL, and every tensor the call could have written still holds its NaN fill."""
    calls = _calls(dev, torch.float32, 8)
    for name, (args, out) in calls.items():
        assert _invoke(name, args, code) == E_INVAL, name
    torch.cuda.synchronize()
    for name, (_, out) in calls.items():
        for k, t in out.items():
            assert bool(torch.isnan(t).all()), f"{name} wrote {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", L_OPS)
def test_L_above_256_is_refused_in_bf16_alone(dev, name):
    """Spike counts up to 256 are exact in bf16: the bf16 form refuses L = 257 and runs L = 256; fp32 runs 257."""
    from aura_snn_rag_amd import _lib
    call = lambda dtype, L, code: _invoke(name, _calls(dev, dtype, L)[name][0], code)
    assert call(torch.bfloat16, 257, _lib.DTYPE_BF16) == E_INVAL
    assert call(torch.bfloat16, 256, _lib.DTYPE_BF16) == _lib.AURA_OK
    assert call(torch.float32, 257, _lib.DTYPE_F32) == _lib.AURA_OK
    torch.cuda.synchronize()


def test_no_bf16_twin_is_declared():
    from aura_snn_rag_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aura_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aura_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 20
    twins = sorted(n for n in declared | set(_lib.SIGNATURES) if n.endswith("_bf16"))
    assert not twins, twins
