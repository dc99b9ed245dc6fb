"""The inverted-list entry points of the C ABI on the host: one function per operation, the image's format an argument
(``AURA_IMAGE_BF16`` / ``AURA_IMAGE_F16``), the recall's layout an ``aura_ivf2_lists`` struct.  Every call below is
refused (or is a no-op) before any launch, so the pointers are fakes that are never dereferenced and no device is
needed: what is checked is that each field and argument reaches the check that the header states for it -- a struct
mirror with a wrong offset, or a prototype with a wrong position, fails here."""
import ctypes

import pytest

P = 0x10000                                               # 256-byte aligned, never dereferenced
OK, INVAL, ALIGN = 0, -1, -3
NS, N, D, NQ, K = 32, 100, 64, 3, 8


@pytest.fixture(scope="module")
def lib():
    from aura_snn_rag_amd import _lib
    return _lib.load()


def _search(lib, fields=(), **kw):
    """aura_knn_search_ivf2 on one valid layout and one valid call, with ``fields`` of the struct and ``kw`` of the
    call replaced."""
    from aura_snn_rag_amd import _lib
    f = dict(bank=P, inv_norm=P, meta=P, centroids=P, image=P, rho=P, sorted_rows=P, pad_off=P, list_len=P,
             lists_flag=None, row_constants=None, n_sorted=NS, N=N, D=D, nprobe=4, image_format=_lib.IMAGE_F16)
    f.update(fields)
    a = dict(lists=None, queries=P, now=1.0, nq=NQ, k=K, probe_ids=None, idx_base=0, out_scores=P, out_idx=P, workspace=P,
             workspace_bytes=None, overflow_out=P, stage=0, k2=0, bounds=None, host_word=None, host_seq=0)
    a.update(kw)
    st = _lib.Ivf2ListsStruct(**f)
    if a["lists"] is None:
        a["lists"] = ctypes.addressof(st)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(lib.aura_knn_ivf2_workspace_bytes(max(f["n_sorted"], 0), max(a["nq"], 0), K), 1)
    return lib.aura_knn_search_ivf2(a["lists"], a["queries"], a["now"], a["nq"], a["k"], a["probe_ids"], a["idx_base"],
                                    a["out_scores"], a["out_idx"], a["workspace"], a["workspace_bytes"], a["overflow_out"],
                                    a["stage"], a["k2"], a["bounds"], a["host_word"], a["host_seq"], None)


def test_the_struct_mirror_has_the_headers_layout():
    from aura_snn_rag_amd import _lib
    S = _lib.Ivf2ListsStruct
    names = [n for n, _ in S._fields_]
    assert names == ["bank", "inv_norm", "meta", "centroids", "image", "rho", "sorted_rows", "pad_off", "list_len",
                     "lists_flag", "row_constants", "n_sorted", "N", "D", "nprobe", "image_format"]
    assert [getattr(S, n).offset for n in names] == [8 * i for i in range(14)] + [112, 116]      # no interior padding
    assert ctypes.sizeof(S) == 120
    assert (_lib.IMAGE_BF16, _lib.IMAGE_F16) == (0, 1)


def test_the_recall_refuses_every_bad_field_and_argument_before_any_launch(lib):
    assert _search(lib, lists=0) == INVAL                                       # NULL struct (0 is not "fill it in")
    for name in ("bank", "inv_norm", "meta", "centroids", "image", "rho", "sorted_rows", "pad_off", "list_len"):
        assert _search(lib, {name: None}) == INVAL, name                        # one at a time: every field's offset
    for name in ("row_constants", "image", "meta", "bank"):
        assert _search(lib, {name: P + 4}) == ALIGN, name
    for fields in (dict(n_sorted=0), dict(n_sorted=24), dict(D=0), dict(D=12), dict(D=776), dict(N=0), dict(nprobe=0),
                   dict(nprobe=9), dict(image_format=2)):
        assert _search(lib, fields) == INVAL, fields
    for kw in (dict(k=0), dict(k=257), dict(stage=-1), dict(stage=5), dict(stage=1, bounds=None),
               dict(stage=1, bounds=P, k2=K + 1), dict(host_word=P, overflow_out=None), dict(host_word=P, stage=1, bounds=P),
               dict(workspace=None), dict(workspace_bytes=0), dict(queries=None), dict(out_scores=None),
               dict(out_idx=None)):
        assert _search(lib, **kw) == INVAL, kw
    assert _search(lib, workspace=P + 16) == ALIGN
    assert _search(lib, queries=P + 4) == ALIGN
    # the order of the refusals: the table's alignment before the format, the format before the stage, both before the
    # sizes; nq == 0 is a no-op before any pointer is looked at
    assert _search(lib, dict(row_constants=P + 4, image_format=2)) == ALIGN
    assert _search(lib, dict(row_constants=P + 4, n_sorted=0)) == ALIGN
    assert _search(lib, nq=0) == OK
    assert _search(lib, dict(bank=None, image=P + 4), nq=0, workspace=None) == OK
    assert _search(lib, dict(image_format=2), nq=0) == INVAL and _search(lib, nq=0, stage=5) == INVAL
    assert _search(lib, dict(image_format=0), nq=0) == OK                      # bf16 is the other valid format


def test_the_writers_and_small_readers_take_the_format_as_an_argument(lib):
    BF16, F16 = 0, 1

    def shadow_sorted(n=16, rho16=None, fmt=F16):
        return lib.aura_bank_shadow_sorted(P, P, P, P, P, rho16, P, n, D, fmt, None)

    def append(n=4, rho16=None, fmt=F16, rowc=None):
        return lib.aura_ivf2_append(P, P, P, P, n, D, P, P, P, P, P, P, rho16, P, rowc, 1.0, fmt, None)

    def row_constants(n=16, fmt=F16, rho=P):
        return lib.aura_ivf2_row_constants(P, rho, P, n, D, 1.0, P, fmt, None)

    def blend(n=4, rho16=None, fmt=F16, image=None):
        return lib.aura_bank_blend(P, P, N, N, D, P, -1, n, P, P, 0.5, P, None, P if image else None, 0, image, rho16,
                                   image, image, NS, fmt, None)

    def find_repeats(n=4, fmt=F16, meta=None, tags=None, n_bank=N, ovf=P):
        nbytes = lib.aura_bank_find_repeats_workspace_bytes(max(n, 1))
        return lib.aura_bank_find_repeats(P, P, n_bank, D, P, None, n_bank, P, P, n, 0.9, P, P, P, ovf, P, nbytes, meta,
                                          tags, fmt, None)

    for fn in (shadow_sorted, append, row_constants, blend, find_repeats):
        assert fn(fmt=2) == INVAL and fn(fmt=-1) == INVAL, fn.__name__
        assert fn(0, fmt=2) == INVAL, fn.__name__                               # the format is checked before n == 0
        assert fn(0, fmt=F16) == OK and fn(0, fmt=BF16) == OK, fn.__name__
    for fn in (shadow_sorted, append, blend):
        assert fn(rho16=P, fmt=BF16) == INVAL, fn.__name__                      # rho16 goes with the half image only
        assert fn(0, rho16=P, fmt=BF16) == INVAL and fn(0, rho16=P, fmt=F16) == OK, fn.__name__
    # the checks behind the format are still there, for both formats
    for fmt in (BF16, F16):
        assert lib.aura_bank_shadow_sorted(P, P, P, P + 4, P, None, P, 16, D, fmt, None) == ALIGN
        assert lib.aura_bank_shadow_sorted(P, P, P, None, P, None, P, 16, D, fmt, None) == INVAL
        assert append(rowc=P + 4, fmt=fmt) == ALIGN
        assert row_constants(rho=None, fmt=fmt) == INVAL
        assert blend(image=P + 4, fmt=fmt) == ALIGN
    assert append(rowc=P, rho16=None, fmt=F16) == INVAL                         # the half image's constants need rho16
    # aura_bank_find_repeats: batch_tags selects the scoped search and its checks; without it meta is ignored
    assert find_repeats(tags=P, meta=None) == INVAL
    assert find_repeats(tags=P + 2, meta=P) == ALIGN and find_repeats(tags=P, meta=P + 2) == ALIGN
    assert find_repeats(ovf=None) == INVAL and find_repeats(0, ovf=None) == INVAL
