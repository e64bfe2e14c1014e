"""The grouped frame-augmentation entry points (include/svla.h: svla_aug_*_grouped) validate the whole host table before they enqueue anything, so what they
refuse they refuse without a GPU: every case below returns SVLA_EINVAL (-1) from host code alone.  (A valid table would go on to the copy and the launch: those
are tests/test_augment_grouped_gpu.py.)  The frame / partials / scratch pointers are never dereferenced by a refused call; they only have to be non-null."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def cdll():
    from safevla_amd import build
    return ctypes.CDLL(build.build())


def _entry(**kw):
    from safevla_amd.ops import AugTransform
    t = AugTransform()
    t.nops, t.ops_packed, t.nops_before_contrast = 4, 0x3210, 1            # brightness, contrast, saturation, hue
    t.f = (ctypes.c_float * 4)(1.1, 0.9, 1.05, 0.01)
    t.wx, t.wy = (ctypes.c_float * 5)(*[0.2] * 5), (ctypes.c_float * 9)(*[1 / 9] * 9)
    t.top, t.left, t.bh, t.bw, t.post_mask, t.sharpen = 1, 1, 14, 14, 0xFE, 1
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _call_all(cdll, table, N=4, H=16, W=16, group_len=2):
    from safevla_amd.ops import AugTransform
    host = (AugTransform * len(table))(*table)
    x, y, part, dev = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(4))
    p = ctypes.cast(host, ctypes.c_void_p)
    return (cdll.svla_aug_gray_partials_grouped(x, N, H, W, group_len, p, dev, part, None),
            cdll.svla_aug_jitter_blur_grouped_u8(x, y, N, H, W, group_len, p, dev, part, None),
            cdll.svla_aug_resize_post_sharp_grouped_u8(x, y, N, H, W, group_len, p, dev, None))


def _header_layout():
    """[(field, dword offset, dwords)] of ``typedef struct svla_aug_transform`` as include/svla.h declares it (every member is an int or a float, so 4 bytes each)"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svla.h")).read()
    body = re.search(r"typedef struct svla_aug_transform \{(.*?)\} svla_aug_transform;", src, flags=re.S).group(1)
    out, at = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        assert ty in ("int", "float"), decl
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", n)
            cnt = int(m.group(2) or 1)
            out.append((m.group(1), at, cnt, ty))
            at += cnt
    return out, at


def test_table_entry_layout_matches_the_header():
    from safevla_amd.ops import AugTransform
    fields, dwords = _header_layout()
    assert dwords == 27 and ctypes.sizeof(AugTransform) == 4 * dwords
    assert [n for n, *_ in fields] == [n for n, _ in AugTransform._fields_]                     # the same members in the same order
    for name, at, cnt, ty in fields:
        f = getattr(AugTransform, name)
        assert (f.offset, f.size) == (4 * at, 4 * cnt), name
        base = dict(AugTransform._fields_)[name]
        elem = base._type_ if issubclass(base, ctypes.Array) else base
        assert elem is (ctypes.c_int if ty == "int" else ctypes.c_float), name
    assert [(n, getattr(AugTransform, n).offset) for n in ("nops", "f", "nops_before_contrast", "wx", "wy", "top", "post_mask", "sharpen")] == \
        [("nops", 0), ("f", 8), ("nops_before_contrast", 24), ("wx", 28), ("wy", 48), ("top", 84), ("post_mask", 100), ("sharpen", 104)]


@pytest.mark.parametrize("bad", [
    dict(nops=5), dict(nops=-1), dict(ops_packed=0x4210), dict(ops_packed=0x13210),      # too many operations, an unknown code, bits beyond the nops codes
    dict(nops_before_contrast=0), dict(nops_before_contrast=-1),                          # not the position of contrast in the order
    dict(bh=16), dict(left=3), dict(top=-1), dict(bw=0),                                  # a box that leaves the image / is empty
    dict(post_mask=0x7F), dict(post_mask=0), dict(post_mask=0x1FE), dict(sharpen=2)], ids=str)
def test_invalid_entry_in_any_group_is_refused(cdll, bad):
    assert _call_all(cdll, [_entry(**bad), _entry()]) == (-1, -1, -1)
    assert _call_all(cdll, [_entry(), _entry(**bad)]) == (-1, -1, -1)                      # in group 1 only


def test_invalid_geometry_is_refused(cdll):
    ok = [_entry(), _entry()]
    assert _call_all(cdll, ok, N=4, group_len=3) == (-1, -1, -1)                           # N % group_len != 0
    assert _call_all(cdll, ok, N=4, group_len=0) == (-1, -1, -1)
    assert _call_all(cdll, ok, N=0) == (-1, -1, -1)
    small = [_entry(top=0, left=0, bh=1, bw=1)] * 2
    assert _call_all(cdll, small, H=4) == (-1, -1, -1) and _call_all(cdll, small, W=2) == (-1, -1, -1)
    no_contrast = [_entry(nops=1, ops_packed=0, nops_before_contrast=-1)] * 2              # valid entries; null pointers are refused
    null = ctypes.c_void_p(0)
    from safevla_amd.ops import AugTransform
    host = (AugTransform * 2)(*no_contrast)
    p, a = ctypes.cast(host, ctypes.c_void_p), ctypes.c_void_p(0x1000)
    assert cdll.svla_aug_resize_post_sharp_grouped_u8(a, a, 4, 16, 16, 2, p, a, None) == -1      # x == y
    assert cdll.svla_aug_resize_post_sharp_grouped_u8(a, ctypes.c_void_p(0x2000), 4, 16, 16, 2, p, null, None) == -1
    assert cdll.svla_aug_resize_post_sharp_grouped_u8(a, ctypes.c_void_p(0x2000), 4, 16, 16, 2, null, a, None) == -1
    assert cdll.svla_aug_gray_partials_grouped(a, 4, 16, 16, 2, p, a, null, None) == -1
