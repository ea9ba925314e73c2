"""Batch G1 multi-scalar multiplication (include/bn254_verify.h: bn254_g1_bases_prepare, bn254_g1_msm_batch, _device, bn254_g1_msm_reserve) without a GPU: the
argument checks of the six entries, the statuses of bn254_g1_bases_prepare for points it refuses, the item length, the limits against the planner of the G1 walk, and
through bn254_dbg_g1_msm_batch(device = -1) -- the HOST compile of the loader (g1msm_load_item), the rows of the plan, the row sum and the store -- every vector class
of tests/g1_msm_common.py against Python integers and the oracle, byte for byte, in the split, the unsplit and the joint form."""
import ctypes as C
import os
import re

import pytest

import g1_msm_common as M
import kzg_common as Z

E_BAD_ARG = -1
NO_SUCH_DEVICE = 4097
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, lane_budget, joint_g, form of a shape with variable terms): a small launch splits by itself; a budget of 64 lanes forces one row per term, joint_g joint rows
FORMS = (("split", 0, 0, "split"), ("unsplit", 64, 0, "unsplit"), ("joint2", 64, 2, "joint"), ("joint8", 64, 8, "joint"))


def _raises_bad_arg(pkg, fn, *a, **kw):
    with pytest.raises(pkg.Bn254Error) as e:
        fn(*a, **kw)
    assert e.value.code == E_BAD_ARG, e.value


def test_vectors_hold_every_class(O):
    """every class exists by name for the shapes it can exist for, all of them over the shapes of this file; more than half of every list is summed to a point other
    than the identity with and without the strict flag, and every status of the definition occurs"""
    seen = set()
    for shape in M.SHAPES:
        bs, bpts, vecs = M.vectors(O, shape)
        names = {x.name for x in vecs}
        for c, exists in M.CLASSES.items():
            assert (c in names) == bool(exists(*shape)), (shape, c)
        seen |= names
        assert {"valid_first", "error_between_valid", "valid_third"} <= names and [x.name for x in vecs[:3]] == ["valid_first", "error_between_valid", "valid_third"]
        assert vecs[0].status(True) == vecs[2].status(True) == M.ACCEPT and vecs[1].status(True) != M.ACCEPT
        for strict in (False, True):
            assert M.summed_share(O, vecs, strict) > 0.5, (shape, strict)
        if shape[0] + shape[1]:
            assert {x.status() for x in vecs} == {M.ACCEPT, M.NOT_MEMBER, M.NOT_ON_CURVE}
        assert len(bpts) == 64 * shape[2] and (shape[2] < 2 or bytes(64) in [bpts[64 * j:64 * j + 64] for j in range(shape[2])])
    assert set(M.CLASSES) <= seen
    for n, k in (("r", M.R), ("lambda", M.LAMBDA), ("2_256_minus_1", 2 ** 256 - 1), ("128bit", None), ("129bit", None)):
        assert "scalar_%s_var" % n in seen and "scalar_%s_shared" % n in seen
    assert dict(M.SCALARS)["128bit"].bit_length() == 128 and dict(M.SCALARS)["129bit"].bit_length() == 129


def test_item_length_and_limits_are_the_headers(pkg):
    text = open(os.path.join(ROOT, "include", "bn254_verify.h")).read()
    body = re.search(r"#define\s+BN254_G1_MSM_ITEM_LEN\(v, u, s\)\s+(.*)", text).group(1)
    expr = body.replace("(size_t)", "")
    for v in range(0, 17):
        for u in range(0, 5):
            for s in range(0, 17):
                assert eval(expr, {"v": v, "u": u, "s": s}) == pkg.g1_msm_item_len(v, u, s) == 96 * v + 64 * u + 32 * s
    lim = {n: int(x) for n, x in re.findall(r"#define\s+BN254_G1_MSM_MAX_(VAR|UNIT|SHARED)\s+(\d+)", text)}
    assert lim == {"VAR": pkg.G1_MSM_MAX_VAR, "UNIT": pkg.G1_MSM_MAX_UNIT, "SHARED": pkg.G1_MSM_MAX_SHARED} == {"VAR": 16, "UNIT": 4, "SHARED": 16}
    assert re.search(r"#define\s+BN254_ABI_VERSION\s+5\b", text)
    # the pass formula of the header
    for shape, items in (((1, 0, 0), 2 ** 18), ((2, 0, 0), 2 ** 18), ((16, 0, 0), 63360), ((16, 4, 16), (2 ** 31 // (105 * 36 + 1792 * 16 + 3522)) // 64 * 64)):
        st = pkg.dbg_g1_msm_batch_state(*shape)
        assert st["formula_items"] == items and st["bytes_per_item"] == 105 * sum(shape) + 1792 * shape[0] + 3522, shape
        assert st["pass_items"] <= st["formula_items"]


def test_every_shape_within_the_limits_plans(pkg):
    """the limits are the planner's own: every shape of 0 .. 16 variable, 0 .. 4 unit and 0 .. 16 shared terms plans at ten sizes, three lane budgets and four joint
    sizes (173 280 plans), the largest plan uses all 32 rows, and one term more of either kind is refused"""
    fn = pkg.lib().bn254_dbg_g1_msm_batch_plan
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    rows = C.c_int(0)
    ref = C.byref(rows)
    plans, most = 0, 0
    for v in range(17):
        for u in range(5):
            for s in range(17):
                if v + u + s == 0:
                    continue
                for n in (64, 128, 1024, 4096, 16384, 16448, 49152, 65536, 131072, 262144):
                    for budget in (64, 65536, 1 << 22):
                        for joint in (0, 2, 4, 8):
                            assert fn(v, u, s, n, budget, joint, ref) == 0, (v, u, s, n, budget, joint)
                            assert 1 <= rows.value <= 32
                            most = max(most, rows.value)
                            plans += 1
    assert plans == 173280 and most == 32
    assert pkg.dbg_g1_msm_batch_plan(17, 0, 0, 64) is None and pkg.dbg_g1_msm_batch_plan(0, 5, 0, 64) is None and pkg.dbg_g1_msm_batch_plan(0, 0, 17, 64) is None
    assert pkg.dbg_g1_msm_batch_plan(1, 0, 0, 64) == 2 and pkg.dbg_g1_msm_batch_plan(2, 1, 0, 64) == 4      # ecMul, and the rows of a KZG opening


def test_argument_checks_come_before_any_device(pkg, O):
    """BN254_E_BAD_ARG on a device ordinal that does not exist, out and status untouched; n == 0 is BN254_OK"""
    L = pkg.lib()
    batch, dev, reserve = L.bn254_g1_msm_batch, L.bn254_g1_msm_batch_device, L.bn254_g1_msm_reserve
    batch.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
    dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    reserve.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    items = bytes(96 * 4)
    out = (C.c_uint8 * 256)(*([0xEE] * 256)); st = (C.c_uint8 * 4)(*([0xEE] * 4))
    D = NO_SUCH_DEVICE
    bad = [
        (items, 96, 1, 0, 0, None, 4, out, st, D, 2),              # BN254_FLAG_RLC is not this entry's
        (items, 96, 1, 0, 0, None, 4, out, st, D, 8),
        (items, 96, 0, 0, 0, None, 4, out, st, D, 0),              # no term
        (items, 4096, 17, 0, 0, None, 1, out, st, D, 0), (items, 4096, 0, 5, 0, None, 1, out, st, D, 0), (items, 4096, 0, 0, 17, None, 1, out, st, D, 0),
        (items, 95, 1, 0, 0, None, 4, out, st, D, 0),              # a stride below the item
        (items, 127, 0, 2, 0, None, 3, out, st, D, 0),
        (items, 96, 0, 0, 1, None, 4, out, st, D, 0),              # shared terms without a handle
        (None, 96, 1, 0, 0, None, 4, out, st, D, 0), (items, 96, 1, 0, 0, None, 4, None, st, D, 0), (items, 96, 1, 0, 0, None, 4, out, None, D, 0),
        (items, 2 ** 63, 1, 0, 0, None, 4, out, st, D, 0),         # n items of that stride overflow the address space
    ]
    for a in bad:
        assert batch(*a) == E_BAD_ARG, a
        d_items = C.cast(C.c_char_p(a[0]), C.c_void_p) if a[0] is not None else None
        assert dev(d_items, *a[1:10], None, a[10]) == E_BAD_ARG, a
    assert bytes(out) == b"\xee" * 256 and bytes(st) == b"\xee" * 4
    # a handle that is none of this library's
    fake = (C.c_uint8 * 64)()
    assert batch(items, 96, 0, 0, 1, C.cast(fake, C.c_void_p), 4, out, st, D, 0) == E_BAD_ARG
    # n == 0: nothing to do, whatever the pointers
    assert batch(None, 96, 1, 0, 0, None, 0, None, None, D, 0) == 0 and dev(None, 96, 1, 0, 0, None, 0, None, None, D, None, 0) == 0
    assert batch(None, 96, 0, 0, 0, None, 0, None, None, D, 0) == E_BAD_ARG      # ... but the shape is checked first
    for shape in ((0, 0, 0), (17, 0, 0), (0, 5, 0), (0, 0, 17)):
        assert reserve(64, *shape, D) == E_BAD_ARG, shape
    assert reserve(64, 1, 0, 0, D) in (-1, -2) and b"device" in L.bn254_last_error().lower()      # a shape that is fine, a device that is not (or none at all)
    # bn254_g1_bases_prepare / _count / _free
    prep, count, free = L.bn254_g1_bases_prepare, L.bn254_g1_bases_count, L.bn254_g1_bases_free
    prep.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    count.argtypes = [C.c_void_p]; count.restype = C.c_size_t
    free.argtypes = [C.c_void_p]; free.restype = None
    h = C.c_void_p(None); s1 = C.c_uint8(0xEE)
    g = O.g1_gen()
    for a in ((None, 1, D, C.byref(h), C.byref(s1)), (g, 0, D, C.byref(h), C.byref(s1)), (g * 17, 17, D, C.byref(h), C.byref(s1)), (g, 1, D, None, C.byref(s1)),
              (g, 1, D, C.byref(h), None)):
        assert prep(*a) == E_BAD_ARG, a
    assert s1.value == 0xEE and not h.value
    assert prep(g, 1, D, C.byref(h), C.byref(s1)) in (-1, -2) and not h.value      # good points, no such device (or none at all)
    assert count(None) == 0 and count(C.cast(fake, C.c_void_p)) == 0
    free(None)
    # the probe
    _raises_bad_arg(pkg, pkg.dbg_g1_msm_batch, items, 1, 0, 0, lane_budget=63)
    _raises_bad_arg(pkg, pkg.dbg_g1_msm_batch, items, 1, 0, 0, joint_g=9)
    _raises_bad_arg(pkg, pkg.dbg_g1_msm_batch, bytes(32 * 4), 0, 0, 1)               # a shared term without a base
    _raises_bad_arg(pkg, pkg.dbg_g1_msm_batch, bytes(32 * 4), 0, 0, 1, base_points=M.be(1) + M.be(3))      # a base off the curve


def test_bases_prepare_refuses_bad_points_without_a_device(pkg, O):
    """the first failure over the points, in order, with no handle and return code BN254_OK -- decided before the device is looked at"""
    g, q = O.g1_gen(), M.g1_of(O, 5)
    off = q[:32] + M.be((int.from_bytes(q[32:], "big") + 1) % M.P)
    for pts, want in ((M.be(M.P) + g[32:], M.NOT_MEMBER), (g[:32] + M.be(2 ** 256 - 1), M.NOT_MEMBER), (off, M.NOT_ON_CURVE), (g + bytes(64) + off, M.NOT_ON_CURVE),
                      (g + off + M.be(M.P) + g[32:], M.NOT_ON_CURVE), (g + M.be(M.P + 1) + M.be(7) + off, M.NOT_MEMBER), (M.be(M.P + 2) + M.be(1), M.NOT_MEMBER)):
        st, h = pkg.g1_bases_prepare(pts, device=NO_SUCH_DEVICE)
        assert st == want and h is None, (want, st)


def _check(pkg, O, shape, strict, form, stride_pad, device=-1, vecs=None, bpts=None):
    name, budget, joint, want_form = form
    if vecs is None:
        _, bpts, vecs = M.vectors(O, shape)
    ilen = pkg.g1_msm_item_len(*shape)
    buf, mem = M.batch(vecs, len(vecs), ilen, ilen + stride_pad)
    r = pkg.dbg_g1_msm_batch(buf, *shape, base_points=bpts, n=len(mem), stride=ilen + stride_pad, flags=pkg.FLAG_STRICT_SCALARS if strict else 0, lane_budget=budget,
                             joint_g=joint, device=device)
    out, st = M.expected(O, mem, strict)
    for i, x in enumerate(mem):
        assert r["status"][i] == st[i], (shape, name, x.name, r["status"][i], st[i])
        assert r["out"][64 * i:64 * i + 64] == out[64 * i:64 * i + 64], (shape, name, x.name)
    assert r["form"] == (want_form if shape[0] else "unsplit") and 1 <= r["rows"] <= 32
    return r


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("shape", M.SHAPES, ids=["%d-%d-%d" % s for s in M.SHAPES])
def test_host_compile_against_the_oracle(pkg, O, shape, form):
    """every vector class of the shape, with and without BN254_FLAG_STRICT_SCALARS, packed and at a padded stride that is no multiple of 4 (the loader's byte path): the
    status bytes are the definition's, the sums the oracle's, an item that ends in an error leaves zero bytes and does not disturb its neighbours"""
    first = None
    for strict in (False, True):
        for pad in (0, 5):
            r = _check(pkg, O, shape, strict, form, pad)
            if not strict:
                assert first is None or (r["out"], r["status"]) == first      # the stride changes nothing
                first = (r["out"], r["status"])
    _, _, vecs = M.vectors(O, shape)
    out, st = M.expected(O, vecs, True)
    assert st[0] == st[2] == M.ACCEPT and st[1] != M.ACCEPT and out[:64] != bytes(64) and out[128:192] != bytes(64)


def test_an_identity_base_alone_contributes_nothing(pkg, O):
    """(0, 0, 1) on a base that is the identity: every sum is the identity, every status ACCEPT, whatever the scalar"""
    items = b"".join(M.be(k) for _, k in M.SCALARS)
    r = pkg.dbg_g1_msm_batch(items, 0, 0, 1, base_points=bytes(64))
    assert r["out"] == bytes(64 * len(M.SCALARS)) and r["status"] == bytes([M.ACCEPT] * len(M.SCALARS))
    r = pkg.dbg_g1_msm_batch(items, 0, 0, 1, base_points=bytes(64), flags=pkg.FLAG_STRICT_SCALARS)
    assert r["status"] == bytes(M.NOT_MEMBER if k >= M.R else M.ACCEPT for _, k in M.SCALARS)


def test_ecadd_and_ecmul_of_eip196(pkg, O):
    """the shapes (0, 2, 0) and (1, 0, 0) on the generator: 1 + 2 = 3, P + (-P) = 0, P + 0 = P, k G with k read modulo r"""
    g = O.g1_gen()
    neg = g[:32] + M.be(M.P - int.from_bytes(g[32:], "big"))
    r = pkg.dbg_g1_msm_batch(g + M.g1_of(O, 2) + g + neg + g + bytes(64) + bytes(128), 0, 2, 0)
    assert r["out"] == M.g1_of(O, 3) + bytes(64) + g + bytes(64) and r["status"] == bytes([M.ACCEPT] * 4)
    r = pkg.dbg_g1_msm_batch(g + M.be(9) + g + M.be(M.R + 9) + g + M.be(M.R) + bytes(64) + M.be(77), 1, 0, 0)
    assert r["out"] == M.g1_of(O, 9) * 2 + bytes(128) and r["status"] == bytes([M.ACCEPT] * 4)


def test_kzg_fold_is_the_shape_2_1_0(pkg, O):
    """what exists already says the same: for the openings of tests/kzg_common.py the items (H, z), (g1, r - y), C give the F_i = C_i - y_i g1 + z_i H_i that
    bn254_dbg_kzg_fold(device = -1) reports"""
    K, vecs = Z.vectors(O)
    st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
    assert st == M.ACCEPT
    mem = [v for v in vecs if v.err is None]
    assert len(mem) >= 20
    fold = pkg.dbg_kzg_fold(key, b"".join(v.rec for v in mem), device=-1)
    items = b"".join(v.rec[64:128] + M.be(v.z) + K["g1"] + M.be((M.R - v.y % M.R) % M.R) + v.rec[0:64] for v in mem)
    r = pkg.dbg_g1_msm_batch(items, 2, 1, 0)
    assert r["status"] == bytes([M.ACCEPT] * len(mem))
    assert r["out"] == fold["f"] and any(r["out"][64 * i:64 * i + 64] == bytes(64) for i in range(len(mem))) and r["out"].count(bytes(64)) < len(mem)
    assert r["out"] == b"".join(Z.g1_of(O, Z.f_scalar(K, v)) for v in mem)
