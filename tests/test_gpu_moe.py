"""The fused MoE zone on the GPU against the fp64 rule of tests/moe_rule.py (``include/aura_hip.h``, "MoE zone").

Every case runs ``ops.moe_forward`` once with the trace and checks, from the kernel's own intermediate results:
  a  ``probs`` within half the bound of fp64; ``indices`` exactly the top k of the kernel's own ``probs`` by the tie rule;
     ``weights`` exactly step 7 on the kernel's own ``probs``;
  b  layer by layer from the kernel's own trace (spikes are integers, so each layer's input is exact): a spike may
     differ from the fp64 rule's only where the fp64 potential is within HALF its bound of a deciding integer, and then
     only to the neighbour; the share of neurons within the whole bound (open) is at most 0.5 %; ``y`` within half the
     bound of fp64 on the kernel's own last spikes;
  c  ``out`` bit-equal to the rule's fp32 sum on the kernel's own ``y`` and ``weights``.
Shapes ``(N, Dm, Hh, E, k, layers, Hr)`` are chosen for the edges: one element; Hh below one MFMA block with P = 66 and
four layers; the workload's widths over 1000 tokens; Dm = 100 and Hh = 40 (no multiple of 8 or 32); 64 experts with
k = 8; Hh at its limit of 512.  Routings forced through the gate: an expert with no token, one with exactly 1, 32 and
33 pairs (tile boundaries), every token on the same two experts.  Inputs: random, rows of zeros, a NaN row, a -inf
and a +inf gate bias, ``attn_gain`` at both clamps.  The worst shares go to the parity record
(``profiles/moe_parity_counts.json``)."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import moe_rule as RULE

pytestmark = pytest.mark.gpu

#        name        N    Dm   Hh   E  k  layers Hr
SHAPES = {"one": (1, 4, 4, 1, 1, 1, 5),
          "small": (33, 8, 12, 3, 2, 4, 37),
          "workload": (1000, 64, 128, 8, 2, 2, 64),
          "ragged": (257, 100, 40, 8, 2, 2, 64),
          "many": (96, 64, 256, 64, 8, 2, 256),
          "wide": (40, 16, 512, 4, 2, 1, 16)}
KINDS = ("random", "zeros", "nan", "neg_inf", "pos_inf", "gain")
CASES = [(s, "random") for s in SHAPES] + [("small", k) for k in KINDS[1:]] + [("ragged", "gain"), ("workload", "nan")]


def _modules(shape, seed=0):
    from aura_snn_rag_amd.core.language_zone.snn_expert import SNNExpert
    from aura_snn_rag_amd.core.liquid_moe import LiquidMoERouter
    N, Dm, Hh, E, k, layers, Hr = shape
    torch.manual_seed(seed)
    router = LiquidMoERouter(Dm, Hr, E, top_k=k)
    with torch.no_grad():
        router.gate_proj.weight.mul_(150.0)
    experts = [SNNExpert(Dm, Hh, Dm, num_layers=layers) for _ in range(E)]
    return router, experts


class Case:
    """One run of the fused ops and everything the checks need, on the host."""

    def __init__(self, dev, shape, kind="random", seed=0, router=None, experts=None, x=None):
        from aura_snn_rag_amd import ops
        N, Dm, Hh, E, k, layers, Hr = shape
        if router is None:
            router, experts = _modules(shape, seed)
        g = torch.Generator().manual_seed(seed + 1)
        if x is None:
            x = torch.randn(N, Dm, generator=g)
        self.gain = None
        if kind == "zeros":
            x[::3] = 0.0
        elif kind == "nan":
            x[N // 2, Dm // 2] = float("nan")
        elif kind == "neg_inf":
            with torch.no_grad():
                router.gate_proj.bias[0] = float("-inf")
        elif kind == "pos_inf":
            with torch.no_grad():
                router.gate_proj.bias[E - 1] = float("inf")
        elif kind == "gain":
            self.gain = torch.cat([torch.full((N // 3,), 1e-3), torch.full((N // 3,), 50.0),
                                   0.25 + 3.0 * torch.rand(N - 2 * (N // 3), generator=g)])
        self.shape, self.x, self.router, self.experts = shape, x, router.to(dev), [e.to(dev) for e in experts]
        c = self.router.cell
        self.route_params = [t.detach() for t in (c.U.weight, c.U.bias, c.W.bias, self.router.gate_proj.weight,
                                                  self.router.gate_proj.bias)]
        lists = [e.fused_parameters() for e in self.experts]
        self.gif = [g_ for _, g_ in lists]
        self.table = ops.moe_expert_table([[t.detach() for t in ts] for ts, _ in lists], self.gif)
        self.params = [[t.detach().cpu().numpy() for t in ts] for ts, _ in lists]
        self.xd = x.to(dev)
        self.gd = None if self.gain is None else self.gain.to(dev)
        self.k = min(k, E)
        self.run = self.forward(self.xd, self.gd, return_trace=True)

    def forward(self, xd, gd=None, **kw):
        from aura_snn_rag_amd import ops
        out, routing, y, trace = ops.moe_forward(xd, *self.route_params, self.table, dt=float(self.router.cell.dt),
                                                 k=self.k, temperature=float(self.router.temperature), attn_gain=gd, **kw)
        return dict(out=out, indices=routing.indices, weights=routing.weights, probs=routing.probs, y=y, trace=trace)

    def host(self):
        return {k: (None if v is None else v.cpu().numpy()) for k, v in self.run.items()}


def _same_bits(a, b):
    """Bit for bit, a NaN matching any NaN (its payload is not part of the rule)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_case(c: Case, name: str):
    N, Dm, Hh, E, k, layers, Hr = c.shape
    k = c.k
    r = c.host()
    x = c.x.numpy()
    gain = None if c.gain is None else c.gain.numpy()
    # ---- a: the router
    r64 = RULE.route64(x, *[t.cpu().numpy() for t in c.route_params], c.router.cell.dt, k, c.router.temperature, gain)
    finite = np.isfinite(r64["probs"]).all(axis=1)
    assert np.isnan(r["probs"][~finite]).all(), "a row that is NaN in the rule is NaN in the kernel"
    share = np.abs(r["probs"][finite].astype(np.float64) - r64["probs"][finite]) / r64["dprobs"][finite]
    p_share = float(share.max()) if share.size else 0.0
    print(f"{name}: worst probs share {p_share:.4f}")
    assert p_share <= 0.5
    order = RULE.topk_order(r["probs"], k)
    assert np.array_equal(r["indices"].astype(np.int64), order)
    assert _same_bits(r["weights"], RULE.weights32(r["probs"], order))
    # ---- b: the experts, layer by layer from the kernel's own trace
    idx = r["indices"]
    neurons = opened = differ = 0
    s_share = y_share = 0.0
    pair_open = np.zeros((N, k), dtype=bool)
    y_bound = np.zeros((N, k, Dm))
    for e in range(E):
        rows, slots = np.nonzero(idx == e)
        if rows.size == 0:
            continue
        a = x[rows]
        ok = np.isfinite(a).all(axis=1)
        for l in range(layers):
            s = r["trace"][rows, slots, l]
            L64 = RULE.layer64(a, *c.params[e][4 * l:4 * l + 4], c.gif[e][l])
            sk = s[ok]
            assert np.array_equal(sk, np.round(sk)) and sk.min(initial=0) >= 0 and sk.max(initial=0) <= c.gif[e][l][1]
            nv, dnv, ref = L64["nv"][ok], L64["dnv"][ok], L64["spikes"][ok]
            away = np.abs(nv - np.clip(np.round(nv), 1, c.gif[e][l][1])) / dnv        # in bounds, from a deciding integer
            mism = sk != ref
            if mism.any():
                s_share = max(s_share, float(away[mism].max()))
                assert (np.abs(sk - ref)[mism] == 1).all(), "an open spike moves to the neighbour only"
            neurons += sk.size
            opened += int(L64["open"][ok].sum())
            differ += int(mism.sum())
            pair_open[rows[ok], slots[ok]] |= L64["open"][ok].any(axis=1)
            a = s
        out = RULE.readout64(a, c.params[e][-2], c.params[e][-1])
        y = r["y"][rows, slots]
        sh = np.abs(y[ok].astype(np.float64) - out["y"][ok]) / out["bound"][ok]
        y_share = max(y_share, float(sh.max()) if sh.size else 0.0)
        y_bound[rows, slots] = out["bound"]
    open_share = opened / max(neurons, 1)
    print(f"{name}: {neurons} neurons, {opened} open ({100 * open_share:.4f} %), {differ} differ from fp64, worst "
          f"spike share {s_share:.4f}, worst y share {y_share:.4f}")
    assert s_share <= 0.5 and y_share <= 0.5 and open_share <= 0.005
    # ---- c: the combine, bit for bit on the kernel's own y and weights
    assert _same_bits(r["out"], RULE.combine32(r["y"], r["weights"], idx))
    helpers.record_parity(f"moe {name}", neurons - differ, neurons, worst_probs_share=p_share, worst_spike_share=s_share,
                          worst_y_share=y_share, open_share=open_share)
    return dict(pair_open=pair_open, y_bound=y_bound, host=r)


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_router_experts_and_combine_against_the_rule(dev, shape, kind):
    c = Case(dev, SHAPES[shape], kind)
    check_case(c, f"{shape}-{kind}")
    if kind == "neg_inf":
        assert not (c.run["indices"] == 0).any() and bool((c.run["probs"][:, 0] == 0).all())
    if kind == "pos_inf":
        assert bool(torch.isnan(c.run["probs"]).all()) and c.run["indices"][0].tolist() == [0, 1]
    if kind == "nan":
        N = SHAPES[shape][0]
        assert bool(torch.isnan(c.run["out"][N // 2]).all()) and bool(torch.isfinite(c.run["out"][:N // 2]).all())


def _forced(dev, group, N=70):
    """E = 5, k = 2: every token takes expert 0; the first ``group`` tokens take expert 1, the others expert 2; experts 3
    and 4 take nobody.  The first hidden unit is dt tanh(50 x_0) = +-dt exactly, and expert 1's logit is 400 times it."""
    shape = (N, 8, 20, 5, 2, 2, 6)
    router, experts = _modules(shape, seed=11)
    with torch.no_grad():
        router.cell.U.weight.zero_(); router.cell.U.bias.zero_(); router.cell.W.bias.zero_()
        router.cell.U.weight[0, 0] = 50.0
        router.gate_proj.weight.zero_()
        router.gate_proj.weight[1, 0] = 400.0
        router.gate_proj.bias.copy_(torch.tensor([10.0, 0.0, 0.0, -20.0, -20.0]))
    x = torch.randn(N, 8, generator=torch.Generator().manual_seed(5))
    x[:, 0] = -1.0
    x[:group, 0] = 1.0
    return Case(dev, shape, router=router, experts=experts, x=x)


@pytest.mark.parametrize("group", [1, 32, 33])
def test_an_expert_with_exactly_this_many_pairs_and_one_with_none(dev, group):
    c = _forced(dev, group)
    counts = torch.bincount(c.run["indices"].flatten().cpu().long(), minlength=5).tolist()
    assert counts == [70, group, 70 - group, 0, 0]
    check_case(c, f"forced-{group}")


def test_every_token_on_the_same_two_experts(dev):
    shape = (100, 8, 20, 6, 2, 2, 6)
    router, experts = _modules(shape, seed=12)
    with torch.no_grad():
        router.gate_proj.weight.zero_()
        router.gate_proj.bias.copy_(torch.tensor([0.0, 0.0, 3.0, 0.0, 0.0, 5.0]))
    c = Case(dev, shape, router=router, experts=experts)
    assert c.run["indices"].tolist() == [[5, 2]] * 100
    check_case(c, "same-two")
    # equal probabilities: the lower id wins
    with torch.no_grad():
        c.router.gate_proj.bias.zero_()
    assert c.forward(c.xd)["indices"].tolist() == [[0, 1]] * 100


def test_first_layer_spikes_equal_gif_run_on_equal_currents(dev):
    """Rows ``alpha e_j`` and W_g = I, b_g = 0 make the kernel's currents known bits: ``fl(fl(alpha W_s[n, j]) + b_s[n])``
    (every other term of both chains is an exact zero).  ``ops.gif_run`` at T = 1 on them gives the kernel's spikes."""
    from aura_snn_rag_amd import ops
    shape = (24, 8, 12, 2, 1, 1, 6)
    router, experts = _modules(shape, seed=13)
    with torch.no_grad():
        for ex in experts:
            ex.layers[0].bias.normal_()
            ex.layers[1].linear.weight.copy_(torch.eye(12))
            ex.layers[1].linear.bias.zero_()
    x = torch.zeros(24, 8)
    alpha = 3.0 + 4.0 * torch.rand(24, generator=torch.Generator().manual_seed(1))
    x[torch.arange(24), torch.arange(24) % 8] = alpha
    c = Case(dev, shape, router=router, experts=experts, x=x)
    for e in range(2):
        rows = torch.nonzero(c.run["indices"][:, 0] == e).flatten().cpu()
        if rows.numel() == 0:
            continue
        ex = c.experts[e]
        W, b = ex.layers[0].weight.detach().cpu(), ex.layers[0].bias.detach().cpu()
        cur = (alpha[rows, None] * W[:, rows % 8].T) + b[None, :]                    # fp32: one rounding each
        h = cur[:, None, :].contiguous().to(dev)
        out = torch.empty_like(h)
        v = torch.zeros(rows.numel(), 12, device=dev)
        theta = torch.full((rows.numel(), 12), float(ex.layers[1].threshold), device=dev)
        n = ex.layers[1]
        ops.gif_run(h, out, v, theta, float(n.decay), int(n.L), float(n.alpha), float(n.threshold), 1)
        assert torch.equal(out[:, 0], c.run["trace"][rows.to(dev), 0, 0])
        assert float(out.max()) >= 1.0, "the currents make spikes"


# ------------------------------------------------------------------------------------------------ d: invariance
@pytest.mark.parametrize("shape", ["small", "ragged"])
def test_a_token_has_the_same_bits_alone_in_any_batch_over_two_calls_and_through_out(dev, shape):
    c = Case(dev, SHAPES[shape], "gain")
    N = SHAPES[shape][0]
    names = ("indices", "weights", "probs", "out")
    same = lambda a, b: all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in names)
    base = {n: c.run[n] for n in names}
    assert same(base, c.forward(c.xd, c.gd))
    res = torch.full_like(c.run["out"], 7.0)
    through = c.forward(c.xd, c.gd, out=res)
    assert through["out"] is res and same(base, through)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2)).to(dev)
    shuffled = c.forward(c.xd[perm].contiguous(), c.gd[perm].contiguous())
    assert same({n: base[n][perm] for n in names}, shuffled)
    for row in (0, N // 2, N - 1):
        alone = c.forward(c.xd[row:row + 1].clone(), c.gd[row:row + 1].clone())
        assert same({n: base[n][row:row + 1] for n in names}, alone)
    head = c.forward(c.xd[:N - 5].clone(), c.gd[:N - 5].clone())
    assert same({n: base[n][:N - 5] for n in names}, head)


def test_a_nan_row_changes_no_other_row(dev):
    c = Case(dev, SHAPES["ragged"], "random")
    bad = c.xd.clone()
    bad[100] = float("nan")
    other = c.forward(bad)
    keep = torch.arange(257, device=dev) != 100
    for n in ("indices", "weights", "probs", "out"):
        assert torch.equal(c.run[n][keep].view(torch.int32), other[n][keep].view(torch.int32)), n
    assert bool(torch.isnan(other["out"][100]).all())


# ------------------------------------------------------------------------------------------------ e: the modules
def _zone(dev, seed=0, **kw):
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    torch.manual_seed(seed)
    args = dict(vocab_size=61, embed_dim=24, hidden_dim=48, num_experts=4, top_k=2, moe_hidden_dim=16)
    args.update(kw)
    zone = MoELanguageZone(**args)
    with torch.no_grad():
        zone.moe_router.gate_proj.weight.mul_(150.0)
    return zone.to(dev)


def test_the_composition_lies_within_twice_the_bound_of_the_fused_experts(dev):
    zone = _zone(dev).eval()
    x = torch.randn(200, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        fused = zone.route_experts(x, return_trace=True)
        comp = zone.route_experts_composed(x, routing=dict(indices=fused.indices, weights=fused.weights, probs=fused.probs))
    experts = [zone.experts[f"expert_{i}"] for i in range(4)]
    case = Case.__new__(Case)
    case.shape, case.k, case.x, case.gain = (200, 16, 24, 4, 2, 2, 64), 2, x.cpu(), None
    case.router, case.experts = zone.moe_router, experts
    c = zone.moe_router.cell
    case.route_params = [t.detach() for t in (c.U.weight, c.U.bias, c.W.bias, zone.moe_router.gate_proj.weight,
                                              zone.moe_router.gate_proj.bias)]
    lists = [e.fused_parameters() for e in experts]
    case.gif = [g for _, g in lists]
    case.params = [[t.detach().cpu().numpy() for t in ts] for ts, _ in lists]
    case.run = dict(out=fused.expert_outputs, indices=fused.indices.int(), weights=fused.weights, probs=fused.probs,
                    y=fused.pair_outputs, trace=fused.trace)
    info = check_case(case, "zone-route-experts")
    r = info["host"]
    settled = ~info["pair_open"].any(axis=1)
    assert settled.sum() > 100
    zero = np.zeros_like(r["weights"], dtype=np.float64)
    bound = RULE.combine64(r["y"], info["y_bound"], r["weights"], zero)["bound"]
    share = np.abs(comp.expert_outputs.cpu().numpy().astype(np.float64) - r["out"].astype(np.float64))[settled] / bound[settled]
    print(f"composition: worst share of twice the bound {share.max() / 2:.4f} over {int(settled.sum())} tokens")
    assert share.max() <= 2.0


def test_forward_without_grad_is_the_composition_of_its_public_parts(dev):
    zone = _zone(dev, seed=4).eval()
    ids = torch.randint(0, 61, (3, 7), generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        torch.manual_seed(21)
        logits, extra = zone(ids)
        on_dev = zone(ids, keep_on_device=True)[1]["probs"]
        torch.manual_seed(21)
        spikes, _ = zone.encoder(zone.embeddings(ids))
        cont = zone.spike_to_continuous(spikes.reshape(21, 1, 48))
        moe = zone.route_experts(cont)
        back = zone.continuous_to_spike(moe.expert_outputs)
        decoded, _ = zone.decoder(back.view(3, 7, back.shape[1], 48).mean(dim=2))
        again = zone.output_proj(decoded)
    assert logits.shape == (3, 7, 61) and torch.equal(logits.view(torch.int32), again.view(torch.int32))
    assert extra["probs"].device.type == "cpu" and on_dev.is_cuda
    assert torch.equal(extra["probs"], moe.probs.view(3, 7, 4).cpu()) and torch.equal(on_dev.cpu(), extra["probs"])


def test_the_recording_path_trains_the_gate_and_every_selected_expert(dev):
    zone = _zone(dev, seed=5).train()
    before = zone.moe_router.expert_usage.clone()
    ids = torch.randint(0, 61, (2, 9), generator=torch.Generator().manual_seed(7)).to(dev)
    logits, _ = zone(ids)
    logits.square().mean().backward()
    assert not torch.equal(zone.moe_router.expert_usage, before), "training updates expert_usage"
    # the Poisson draw of the second bridge is a comparison: as in the reference, forward's loss trains what follows it
    g = zone.output_proj.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    cont = torch.randn(30, 16, device=dev)
    out = zone.route_experts(cont)
    zone.zero_grad()
    out.expert_outputs.square().sum().backward()
    g = zone.moe_router.gate_proj.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    for i in set(out.indices.flatten().tolist()):
        grad = zone.experts[f"expert_{i}"].readout.weight.grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0, i
    for p in zone.parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all())


def test_each_refusal_on_the_device_raises_without_a_launch(dev):
    from aura_snn_rag_amd import _lib, ops
    c = Case(dev, SHAPES["small"])
    with pytest.raises(ops.AuraDeviceError):
        ops.moe_route(c.x, *c.route_params, dt=0.02, k=2)
    routing = ops.moe_route(c.xd, *c.route_params, dt=0.02, k=2)
    with pytest.raises(ValueError):
        ops.moe_experts(c.xd[:10].clone(), routing, c.table)                       # another number of rows
    lib = _lib.load()
    for N, E, k in ((0, 1, 1), (1, 1, 1), (33, 3, 2), (1000, 8, 2), (96, 64, 8)):
        assert lib.aura_moe_workspace_bytes(N, E, k) == ops.moe_workspace_bytes(N, E, k)
    assert lib.aura_moe_workspace_bytes(33, 65, 2) == -1 and lib.aura_moe_workspace_bytes(33, 3, 4) == -1
    # null pointers and bad geometry are refused by the C entry points themselves
    p = c.xd.data_ptr()
    ws = routing.plan
    assert lib.aura_moe_route(None, 33, 8, p, p, p, 37, 0.02, p, p, 3, 2, 1.0, None, p, p, p, ws.data_ptr(), ws.numel(),
                              None) == -1
    assert lib.aura_moe_route(p, 33, 6, p, p, p, 37, 0.02, p, p, 3, 2, 1.0, None, p, p, p, ws.data_ptr(), ws.numel(),
                              None) == -1
    assert lib.aura_moe_route(p, 33, 8, p, p, p, 37, 0.02, p, p, 3, 2, 1.0, None, p, p, p, ws.data_ptr(), 16, None) == -1
    assert lib.aura_moe_experts(p, 33, 8, 12, 4, 3, 2, None, p, p, p, p, p, None, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.aura_moe_experts(p, 33, 8, 10, 4, 3, 2, p, p, p, p, p, p, None, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.aura_moe_experts(p, 33, 8, 12, 5, 3, 2, p, p, p, p, p, p, None, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.aura_moe_experts(p + 4, 33, 8, 12, 4, 3, 2, p, p, p, p, p, p, None, ws.data_ptr(), ws.numel(), None) == -3
