"""The list-sorted image of the inverted lists in IEEE half (image_format = AURA_IMAGE_F16 in the writers and readers):
the rigorous bound on rows and queries built to round the worst way, recall through the half image against the fp32
lists and the fp32 scan (rows and score bits), and the image's upkeep by appends and blends.

The conversion rule's host model is tests/half_image_rule.py (tested on the CPU in test_host_half_image.py); here the
kernels' bits are compared with it."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate as RC
from tests import half_image_rule as R

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _norms(ops, bank):
    inv = torch.empty(bank.shape[0], device=bank.device)
    ops.bank_row_norms(bank, inv, 0, bank.shape[0])
    return inv


# ------------------------------------------------------------------------------------------------------- the bound
def _midpoint_rows(n, D, g, up):
    """Unit rows whose first D-1 coordinates sit just above (below) a HALF rounding midpoint -- 0.125 (1 + 2^-11) lies
    halfway between 0.125 and its successor -- so that round-to-nearest moves every one of them by almost the full
    half ulp in the same direction."""
    a = 0.125 * (1.0 + 2.0 ** -11 + (2.0 ** -16 if up else -2.0 ** -16))
    sign = torch.where(torch.rand(n, D, generator=g) < 0.5, -1.0, 1.0)
    x = sign * a
    rest = 1.0 - (D - 1) * a * a
    assert rest > 0
    x[:, -1] = sign[:, -1] * rest ** 0.5
    return x.float()


def _tiny_rows(n, D, g):
    """Unit rows with 24 elements inside (0, 2^-14) (both signs; stored as 0), four at exactly +-2^-14 and the rest of
    equal magnitude: the subnormal rule at work, and its boundary."""
    x = torch.empty(n, D)
    sign = torch.where(torch.rand(n, D, generator=g) < 0.5, -1.0, 1.0)
    x[:, :24] = 2.0 ** -14 * (0.02 + 0.97 * torch.rand(n, 24, generator=g))
    x[:, 24:28] = 2.0 ** -14
    rest = 1.0 - (x[:, :28].double() ** 2).sum(1)
    x[:, 28:] = (rest / (D - 28)).sqrt().float()[:, None]
    return (sign * x).float()


def test_bound_holds_on_adversarial_half_roundings(dev):
    """The fp16 twin of test_gpu_bank_r02.test_bound_holds_on_adversarial_roundings: D = 64, 9600 rows; rows on half
    rounding midpoints in both directions and rows with elements in (0, 2^-14) and at exactly 2^-14; the queries are
    those rows.  |cos_image - cos_true| <= rho16 + eq (1 + rho16) + e_fix elementwise against fp64."""
    from aura_snn_rag_amd import ops
    D = 64
    g = torch.Generator().manual_seed(0)
    rows = torch.cat([_midpoint_rows(300, D, g, up=False), _midpoint_rows(300, D, g, up=True), _tiny_rows(300, D, g),
                      torch.randn(8700, D, generator=g)])
    N = rows.shape[0]
    assert N == 9600
    bank = rows.to(dev).contiguous()
    inv = _norms(ops, bank)
    ident = torch.arange(N, dtype=torch.int32, device=dev)
    image = torch.full((N, D), float("nan"), dtype=torch.float16, device=dev)
    rho = torch.zeros(N, device=dev); rho16 = torch.zeros(N, device=dev)
    ops.bank_shadow_sorted(bank, inv, ident, image, rho, None, N, rho16=rho16)
    # the image: the host model's bits of fl(bank * inv), no subnormal pattern, no negative zero
    xn = bank * inv.unsqueeze(1)
    want = torch.from_numpy(R.half_bits(xn.cpu().numpy()).view(np.int16))
    got = _bits16(image).cpu()
    assert torch.equal(got, want), "the image is not the rule's bits"
    b = got.numpy().view(np.uint16)
    assert not (((b >> 10) & 0x1F == 0) & (b & 0x3FF != 0)).any(), "a subnormal bit pattern in the image"
    assert not (b == 0x8000).any()
    flushed = (b[600:900] == 0).sum(1)
    assert flushed.min() >= 24, "the tiny elements must be stored as 0"
    assert ((b[600:900] & 0x7FFF) == 0x0400).any(), "no element landed on exactly 2^-14"
    # rho: still the bf16 residual, bit for bit what the row-ordered shadow's kernel writes
    shadow, rho_bf = ops.make_shadow(bank, inv)
    assert torch.equal(_bits32(rho), _bits32(rho_bf)), "rho must stay bank_shadow_update's bits"
    # rho16: the formula on the half residual.  The kernel sums D squares in fp32 (relative error <= D 2^-24 on the sum,
    # half of that after the root, a few ulp for the rest), the model in fp64: 4e-6 relative covers D = 64
    model = torch.from_numpy(R.rho16(xn.cpu().numpy(), D)).float().to(dev)
    assert bool(((rho16 - model).abs() <= 4e-6 * model + 1e-9).all())
    # its worst case: 2^-11 relative on what stays normal (||x|| <= 1.00001) plus the SUBNORMAL TERM sqrt(n_0) 2^-14,
    # n_0 = elements stored as 0, each of which errs by itself, < 2^-14 -- at most sqrt(D) 2^-14 for any row, and
    # nothing for a row without such elements
    c = (0.5 * D + 3) * 2.0 ** -24
    assert float(rho16.max()) <= 1.001 * (2.0 ** -11 * 1.00001 + D ** 0.5 * 2.0 ** -14) + c
    n0 = torch.from_numpy((b == 0).sum(1)).to(dev).float()
    assert bool((rho16 <= 1.001 * (2.0 ** -11 * 1.00001 + n0.sqrt() * 2.0 ** -14) + c).all())
    assert float(rho16[:600].max()) <= 1.001 * 2.0 ** -11 * 1.00001 + c
    assert float(rho16[:600].min()) > 0.9 * 2.0 ** -11, "the midpoint rows must come close to the worst case"
    # three more significand bits: an eighth of the bf16 residual on ordinary rows (the random ones)
    assert float(rho16[900:].mean()) < 0.2 * float(rho[900:].mean()), "the half band is not several times narrower"
    # the bound, elementwise, queries = the adversarial rows themselves
    q = bank[:900]
    qn = q * (1.0 / q.norm(dim=1, keepdim=True))
    qh = torch.from_numpy(R.half_values(qn.cpu().numpy())).to(dev)
    eq = (qh - qn).norm(dim=1) * 1.001 + c
    cos_image = (qh.double() @ image.double().t()).float()
    cos_true = ((q.double() / q.double().norm(dim=1, keepdim=True)) @
                (bank.double() / bank.double().norm(dim=1, keepdim=True)).t()).float()
    err = (cos_image - cos_true).abs()
    e_fix = 2 * D * 2.0 ** -24 + 1e-5
    bound = rho16.unsqueeze(0) + eq.unsqueeze(1) * (1 + rho16.unsqueeze(0)) + e_fix
    print(f"max err {float(err.max()):.3e}, min slack {float((bound - err).min()):.3e}, rho16 max {float(rho16.max()):.3e}")
    assert bool((err <= bound).all()), f"bound violated by {(err - bound).max().item():.3e}"
    # end to end over this bank: one list, the half image == the fp32 scan
    meta = torch.zeros(N, 4, device=dev); meta[:, 0] = 1.0; meta[:, 1] = NOW
    meta[::3, 0] = -0.7                                                   # negative strengths: coarse_eq_worst_f16
    cent = torch.zeros(256, D, device=dev); cent[0] = bank.mean(0); cent[1:] = 1e3
    st = ops.build_ivf2(bank, inv, meta[:, 2])
    qq = torch.cat([q[::7], q[::11] + 0.002 * torch.randn(q[::11].shape, generator=g).to(dev)]).contiguous()
    for k in (1, 5, 40):
        s0, i0 = ops.knn_search(bank, inv, meta, qq, k, NOW, fp32_scan=True)
        s1, i1, o1 = ops.knn_search_ivf2(bank, inv, meta, qq, k, NOW, cent, 8, st["sorted_bf16"], st["rho"],
                                         st["sorted_rows"], st["pad_off"], st["list_len"], n_sorted=st["n_sorted"],
                                         rho16=st["rho16"])
        assert int(o1.item()) & ~ops.KNN_FLAG_NO_CANDIDATES == 0
        assert torch.equal(i0, i1) and torch.equal(s0, s1)


# ---------------------------------------------------------------------------------------------------- end to end
def _lists_of(meta_dev, N):
    cids = meta_dev[:N, 2].to(torch.int32)
    order = torch.sort(cids, stable=True).indices.to(torch.int32).contiguous()
    valid = cids >= 0
    lens = torch.bincount(cids.clamp(min=0).long(), weights=valid.float(), minlength=256)[:256].to(torch.int32).contiguous()
    n_neg = (N - valid.sum()).to(torch.int32).reshape(1)
    off = torch.cat([n_neg, n_neg + torch.cumsum(lens, 0).to(torch.int32)]).contiguous()
    return order, off, lens


@pytest.mark.parametrize("ncent", [60, 256])
@pytest.mark.parametrize("D", [8, 40, 64, 768])
@pytest.mark.parametrize("N", [8192, 20_000])
def test_recall_through_the_half_image(dev, N, D, ncent):
    """Inverted-list recall through the half image == aura_knn_search_ivf (fp32 lists) == the fp32 scan, rows and score
    bits, for nq in {1, 17, 300} x k in {1, 5, 40}: strengths of both signs and zero, a timestamp in the future of
    `now`, a list shorter than 16 rows, rows without a list."""
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(N + 31 * D + ncent)
    centres = torch.randn(64, D, generator=g)
    x = centres[torch.randint(0, 64, (N,), generator=g)] + 0.4 * torch.randn(N, D, generator=g)
    bank = x.to(dev).contiguous()
    inv = _norms(ops, bank)
    meta = torch.zeros(N, 4)
    meta[:, 0] = 0.3 + 0.7 * torch.rand(N, generator=g)
    meta[::5, 0] *= -1.0                                                  # negative strengths
    meta[::17, 0] = 0.0                                                   # ... and zero
    meta[:, 1] = NOW - 7200 * torch.rand(N, generator=g)
    meta[3::101, 1] = NOW + 3000.0                                        # stamped in the future of `now`
    meta = meta.to(dev).contiguous()
    cent = torch.zeros(256, D, device=dev)
    cent[:ncent] = bank[torch.randint(0, N, (ncent,), generator=g).to(dev)]
    cid = ops.kmeans_assign(bank, cent, N, ncent).float()
    c0 = int(cid[0].item())                                               # this list keeps 5 rows: shorter than a tile
    members = torch.nonzero(cid == c0).flatten()
    cid[members[5:]] = -1.0
    cid[1::97] = -1.0
    meta[:, 2] = cid
    order, off, lens = _lists_of(meta, N)
    assert 1 <= int(lens[c0]) <= 5
    st = ops.build_ivf2(bank, inv, meta[:, 2], slack=16 if D == 40 else 0)
    assert st["sorted_bf16"].dtype == torch.float16 and st["rho16"] is not None
    assert float(st["rho16"].max()) < 1.001 * (2.0 ** -11 * 1.00001 + D ** 0.5 * 2.0 ** -14) + (0.5 * D + 3) * 2.0 ** -24
    lists = ops.Ivf2Lists(bank, inv, meta, cent, 8, st["sorted_bf16"], st["rho"], st["sorted_rows"], st["pad_off"],
                          st["list_len"], st["n_sorted"], None, None, st["rho16"])
    qsrc = torch.cat([members[:1].cpu(), torch.randint(0, N, (299,), generator=g)]).to(dev)   # query 0: the short list's
    qall = (bank[qsrc] + 0.3 * bank.std() * torch.randn(300, D, generator=g).to(dev)).contiguous()
    cap_rows = int(torch.topk(lens, 8).values.sum().item())
    for nq in (1, 17, 300):
        q = qall[:nq].contiguous()
        for k in (1, 5, 40):
            s1, r1, o1 = lists.search(q, k, NOW)
            flag = int(o1.item()) & ~ops.KNN_FLAG_NO_CANDIDATES
            s0, r0 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, fp32_scan=True)
            assert flag == 0, f"nq={nq} k={k}: flag {flag}"
            assert torch.equal(r0, r1) and torch.equal(s0, s1), f"nq={nq} k={k}: differs from the fp32 scan"
            cap = ops.ivf_capacity(cap_rows, k)
            assert cap is not None
            s2, r2, o2 = ops.knn_search_ivf(bank, inv, meta, q, k, NOW, N, cent, 8, order, off, lens, cap)
            assert int(o2.item()) == 0
            assert torch.equal(r2, r1) and torch.equal(s2, s1), f"nq={nq} k={k}: differs from the fp32 lists"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_call_form_through_the_one_entry_point(dev, dtype):
    """aura_knn_search_ivf2 is one function: plain, with the caller's probes, with a completion word and in stages it
    gives the same rows and score bits on a half and on a bf16 image -- and probes that the caller FORCES to lists 0..3
    are obeyed, which no other case notices if the function drops ``probe_ids``.  N = 4096, D = 64, 256 centroids drawn
    from the bank, strengths of both signs, nq = 33 (not a multiple of 4 or 32), k = 8, nprobe = 4."""
    from aura_snn_rag_amd import ops
    N, D, nq, k, nprobe = 4096, 64, 33, 8, 4
    g = torch.Generator().manual_seed(5)
    bank = torch.randn(N, D, generator=g).to(dev).contiguous()
    inv = _norms(ops, bank)
    meta = torch.zeros(N, 4)
    meta[:, 0] = 0.3 + 0.7 * torch.rand(N, generator=g)
    meta[::5, 0] *= -1.0
    meta[:, 1] = NOW - 7200 * torch.rand(N, generator=g)
    meta = meta.to(dev).contiguous()
    cent = bank[torch.randperm(N, generator=g)[:256].to(dev)].contiguous()
    meta[:, 2] = ops.kmeans_assign(bank, cent, N, 256).float()
    assert int((meta[:, 2] < 4).sum()) >= k, "lists 0..3 must hold at least k rows"
    st = ops.build_ivf2(bank, inv, meta[:, 2], dtype=dtype)
    assert st["sorted_bf16"].dtype == dtype and (st["rho16"] is None) == (dtype == torch.bfloat16)
    lists = ops.Ivf2Lists(bank, inv, meta, cent, nprobe, st["sorted_bf16"], st["rho"], st["sorted_rows"], st["pad_off"],
                          st["list_len"], st["n_sorted"], None, None, st["rho16"])
    q = bank[torch.randint(0, N, (nq,), generator=g).to(dev)] + 0.3 * torch.randn(nq, D, generator=g).to(dev)
    q = q.contiguous()

    def same(res, what):
        assert torch.equal(res[1], ref[1]) and torch.equal(res[0], ref[0]), what
        assert int(res[2].item()) == 0, what

    s0, r0 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=nprobe, fp32_scan=True)
    ref = lists.search(q, k, NOW)
    ref = (ref[0].clone(), ref[1].clone(), ref[2].clone())
    assert torch.equal(ref[1], r0) and torch.equal(ref[0], s0), "the plain call differs from the fp32 scan"
    assert int(ref[2].item()) == 0
    same(lists.search(q, k, NOW, probe_ids=ops.centroid_probe(q, cent, nprobe)), "the caller's own probes")
    word = ops.CompletionWord(dev)
    res = lists.search(q, k, NOW, word=word)
    assert word.wait() == int(res[2].item())
    same(res, "with a completion word")
    p = lists.staged(q, k, NOW)
    b = p.stage1(k2=k)
    b2 = p.stage2_bounds(b[:, 0].contiguous(), k)
    same(p.stage3(b2[:, 0].contiguous()), "staged on its own bounds")
    forced = torch.full((nq, 8), -1, dtype=torch.int32, device=dev)
    forced[:, :4] = torch.arange(4, dtype=torch.int32, device=dev)
    sf, rf, of = lists.search(q, k, NOW, probe_ids=forced)
    assert int(of.item()) == 0 and bool((rf >= 0).all())
    assert bool((meta[rf.long().flatten(), 2] < 4).all()), "a row from a list that was not probed"
    assert bool((rf != ref[1]).any(dim=1).any()), "forced probes changed nothing"


def test_fuzz_sweep_once(dev):
    """tests/fuzz_ivf2.py unchanged, once: its lists are built by build_ivf2, i.e. in half."""
    from tests import fuzz_ivf2
    assert fuzz_ivf2.sweep(cases=3, seed=3, dev=dev, verbose=True) == 0


# -------------------------------------------------------------------------------------------------------- upkeep
def _rebuilt(ops, bank, inv, st):
    """The image, rho16 and rho a from-scratch bank_shadow_sorted leaves on copies for the layout of ``st``."""
    img = torch.zeros_like(st["sorted_bf16"])
    rho = torch.zeros_like(st["rho"]); rho16 = torch.zeros_like(st["rho16"])
    ops.bank_shadow_sorted(bank, inv, st["sorted_rows"], img, rho, None, st["n_sorted"], rho16=rho16)
    return img, rho, rho16


def test_append_and_blend_keep_image_and_rho16(dev):
    from aura_snn_rag_amd import ops
    D, N, M = 768, 9000, 9600
    g = torch.Generator().manual_seed(11)
    bank = torch.zeros(M, D); bank[:N] = torch.randn(N, D, generator=g)
    bank = bank.to(dev).contiguous()
    inv = torch.ones(M, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    meta = torch.zeros(M, 4, device=dev); meta[:, 0] = 1.0; meta[:, 1] = NOW
    meta[:N, 2] = torch.randint(-20, 256, (N,), generator=g).clamp(min=-1).float().to(dev)
    rho = torch.zeros(M, device=dev)
    st = ops.build_ivf2(bank[:N], inv[:N], meta[:N, 2], slack=32, max_rows=M)
    # (build_ivf2 sizes its per-row arrays by the bank it is given: rebuild them over all M rows)
    st["pos_of_row"] = torch.full((M,), -1, dtype=torch.int32, device=dev)
    st["rho"], st["rho16"] = rho, torch.zeros(M, device=dev)
    ops.bank_shadow_sorted(bank, inv, st["sorted_rows"], st["sorted_bf16"], rho, st["pos_of_row"], st["n_sorted"],
                           rho16=st["rho16"])
    ns = st["n_sorted"]
    rowc = torch.empty(st["sorted_rows"].numel(), 4, device=dev)
    ops.ivf2_row_constants(meta, st["rho16"], st["sorted_rows"], ns, D, NOW, rowc, half=True)

    # ---- append: 200 new rows and 100 overwritten ones
    slots = torch.cat([torch.arange(N, N + 200), torch.randperm(N, generator=g)[:100]]).to(dev)
    bank[slots] = torch.randn(300, D, generator=g).to(dev)
    bank[slots[:7], :40] = 1e-7                                           # elements that the rule stores as 0
    meta[slots, 2] = torch.randint(0, 256, (300,), generator=g).float().to(dev)
    ops.bank_row_norms(bank, inv, 0, M)                                   # (unchanged rows keep their bits)
    ops.ivf2_append(bank, inv, meta, slots, st["sorted_bf16"], st["sorted_rows"], st["pad_off"], st["list_len"],
                    st["pos_of_row"], rho, st["flag"], row_constants=rowc, row_constants_now=NOW, rho16=st["rho16"])
    assert int(st["flag"].item()) == 0
    img2, rho2, rho16_2 = _rebuilt(ops, bank, inv, st)
    listed = st["sorted_rows"][:ns][st["sorted_rows"][:ns] >= 0].long()
    live = st["sorted_rows"][:ns] >= 0                                     # a hole keeps its old bits; it is never scored
    assert torch.equal(_bits16(st["sorted_bf16"][:ns][live]), _bits16(img2[:ns][live])), "append: not the rebuilt image"
    assert torch.equal(_bits32(st["rho16"][listed]), _bits32(rho16_2[listed])), "append: not the rebuilt rho16"
    rho_upd = torch.zeros(M, device=dev)
    sh = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
    ops.bank_shadow_update(bank, inv, sh, rho_upd, 0, N + 200)
    assert torch.equal(_bits32(rho[listed]), _bits32(rho_upd[listed])), "append: rho is not bank_shadow_update's"
    rowc2 = torch.empty_like(rowc)
    ops.ivf2_row_constants(meta, st["rho16"], st["sorted_rows"], ns, D, NOW, rowc2, half=True)
    assert torch.equal(_bits32(rowc[:ns]), _bits32(rowc2[:ns])), "append: the cached row constants went stale"
    with pytest.raises(ValueError):                                       # the half table cannot follow without rho16
        ops.ivf2_append(bank, inv, meta, slots[:1], st["sorted_bf16"], st["sorted_rows"], st["pad_off"], st["list_len"],
                        st["pos_of_row"], rho, st["flag"], row_constants=rowc, row_constants_now=NOW)

    # ---- blend: 64 batch rows repeat 32 held rows
    count = N + 200
    targets = torch.randperm(count, generator=g)[:32].to(torch.int32)
    stored = targets.repeat(2).to(dev)
    leader = torch.full((64,), -1, dtype=torch.int32, device=dev)
    feats = (bank[stored.long()] + 0.05 * torch.randn(64, D, generator=g).to(dev)).contiguous()
    out = feats.clone()
    before16 = st["rho16"].clone()
    ops.bank_blend(bank, inv, count, stored, leader, 0.3, feats=feats, out=out, rho=rho, sorted_bf16=st["sorted_bf16"],
                   sorted_rows=st["sorted_rows"], pos_of_row=st["pos_of_row"], n_sorted=ns, rho16=st["rho16"])
    img3, rho3, rho16_3 = _rebuilt(ops, bank, inv, st)
    assert torch.equal(_bits16(st["sorted_bf16"][:ns][live]), _bits16(img3[:ns][live])), "blend: not the rebuilt image"
    assert torch.equal(_bits32(st["rho16"][listed]), _bits32(rho16_3[listed])), "blend: not the rebuilt rho16"
    ops.bank_shadow_update(bank, inv, sh, rho_upd, 0, count)
    assert torch.equal(_bits32(rho[listed]), _bits32(rho_upd[listed])), "blend: rho is not bank_shadow_update's"
    moved = targets.long().to(dev)
    in_lists = st["pos_of_row"][moved] >= 0
    assert int(in_lists.sum()) > 16 and bool((st["rho16"][moved[in_lists]] != before16[moved[in_lists]]).any())
    # a call without rho16 still keeps the image and rho current
    feats2 = (bank[stored.long()] + 0.05 * torch.randn(64, D, generator=g).to(dev)).contiguous()
    ops.bank_blend(bank, inv, count, stored, leader, 0.3, feats=feats2, out=feats2.clone(), rho=rho,
                   sorted_bf16=st["sorted_bf16"], sorted_rows=st["sorted_rows"], pos_of_row=st["pos_of_row"], n_sorted=ns)
    img4, _, _ = _rebuilt(ops, bank, inv, st)
    assert torch.equal(_bits16(st["sorted_bf16"][:ns][live]), _bits16(img4[:ns][live]))


def test_find_repeats_on_the_half_image_equals_the_dense_path(dev):
    """The shapes of test_gpu_consolidate's sorted_image case (D = 768, 20 000 rows, batches of 256 / 1024 / 64, tau
    0.9 / 0.95): the scan over the list-sorted half image reports what the dense fp32 scan reports, for every row the
    fp64 rule decides by more than the two paths' tolerance."""
    from aura_snn_rag_amd import ops
    D, N = 768, 20_000
    g = torch.Generator().manual_seed(7)
    groups = torch.randn(480, D, generator=g)
    feats = torch.cat([groups.repeat_interleave(6, 0) + 0.05 * torch.randn(2880, D, generator=g),
                       torch.randn(N - 2880, D, generator=g)])[torch.randperm(N, generator=g)].contiguous()
    bank = feats.to(dev)
    inv = _norms(ops, bank)
    cids = torch.randint(-10, 256, (N,), generator=g).clamp(min=-1).float().to(dev)
    cids[cids < 0] = 3.0                                                  # every held row must be in the image
    st = ops.build_ivf2(bank, inv, cids, slack=16)
    tol = RC.tolerance(D)
    for n, seed in ((256, 5), (1024, 6), (64, 7)):
        gb = torch.Generator().manual_seed(seed)
        src = torch.randint(0, N, (n,), generator=gb)
        s = torch.rand(n, 1, generator=gb)
        batch = feats[src] + s * feats[src].norm(dim=1, keepdim=True) / D ** 0.5 * torch.randn(n, D, generator=gb)
        batch[::7] = feats[src[::7]] * 1.25
        batch[3::11] = torch.randn(len(batch[3::11]), D, generator=gb)
        batch[5] = 0.0
        batch = batch.contiguous()
        cs, cb = RC.cosines(bank, inv, N, batch)
        for tau in (0.9, 0.95):
            dense = ops.find_repeats(bank, inv, N, batch.to(dev), tau)[3].cpu()
            half = ops.find_repeats(bank, inv, N, batch.to(dev), tau, image=st["sorted_bf16"],
                                    image_rows=st["sorted_rows"], n_image=st["n_sorted"], rho=st["rho"],
                                    rho16=st["rho16"])[3].cpu()
            assert int(half[3 * n]) == 0 and int(dense[3 * n]) == 0
            und = RC.undecided(cs, cb, tau, tol)
            taint = und.clone()
            near = cb >= tau - tol
            for i in range(n):                                            # an undecided row taints who could repeat it
                if not taint[i] and bool((near[i, :i] & taint[:i]).any()):
                    taint[i] = True
            ok = ~taint
            assert int(taint.sum()) <= max(2, 0.02 * n), "the batch decides too little to compare the paths"
            assert torch.equal(half[:n][ok], dense[:n][ok]) and torch.equal(half[n:2 * n][ok], dense[n:2 * n][ok])
            assert int((half[:n] >= 0).sum()) > n // 10
            RC.replay_check(cs, cb, tau, tol, half[:n], half[n:2 * n], half[2 * n:3 * n].view(torch.float32),
                            bad=RC.degenerate(batch))
