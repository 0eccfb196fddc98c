"""Range of the ping-pong flip kernel's one-reciprocal gate tail (csrc/split_pp.h: SplitPP<.., GSTATE, MERGED>), restated in NumPy.
TEST INFRASTRUCTURE ONLY.

The step with Eu = exp2(a_u), Ec = exp2(a_c), g' = [g (1 + Ec) + Eu] / [(1 + Eu)(1 + Ec)] needs a finite denominator in float32, so the
packer writes one word into the g-state image: 1 iff, for every unit, A_u + A_c <= 120, where (layout: csrc/split_core.h, MODE 2)

    A_u = max over the input spin of |CI[sigma][u row]| + sum over the row's K entries of |w1 + w2 + w3|
    A_c = max over the input spin of |XC[sigma][unit]| + max over the input spin of |CI[sigma][q row]| + the q row's absolute sum

are taken from the image in h (|h| <= 1 there is g in [0, 1] in the g form).  `decode` reads an image as the layout describes it, without
the library; `bounds` restates A_u, A_c per lane entry; `merged32` / `two_rcp32` / `exact64` restate one gate tail.

Rows: lane half hh of a wave owns, for its chain, entry e < 16: unit rows (tile gate, register e) of the full block, gate = 0 r, 1 u,
2 q; entry 16 + j, j < RJ = 9: slot gate RJ + j of the two mixed tiles (tile 3 + slot // 16, register slot % 16).  Register rho of lane
half hh is row r32 = (rho & 3) + 4 hh + 8 (rho >> 2) of the tile."""
import ctypes as C

import numpy as np

NF32, RJ = 1, 9                       # the one kernel row of 37..50 units (csrc/shapes.h: SplitKernels)
NU = 16 * NF32 + RJ
LIMIT = 120.0
LAYOUT_NAMES = ("NT", "NQ", "NUP", "NOUT", "OFF_ASP", "OFF_CI", "OFF_XC", "OFF_WD", "OFF_BD", "BYTES")
RANGE_SLOT = 3                        # word of the head-bias block that holds the verdict


def flat_params(prm):
    return np.concatenate([np.asarray(prm[k], dtype=np.float64).ravel() for k in sorted(prm, key=lambda s: s.encode())])


def images(units, prm):
    """(image in h, image in g, layout) as the host packer builds them"""
    from rnnwavefunctions_amd import _lib
    lib = _lib.load_library()
    flat = flat_params(prm)
    cap = 1 << 18
    ih, ig = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    lay = np.zeros(10, dtype=np.int32)
    rc = lib.rnnwf_host_split_images(units, flat.ctypes.data_as(C.POINTER(C.c_double)), flat.size, ih.ctypes.data, ig.ctypes.data, cap,
                                     lay.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.rnnwf_last_error(None).decode()
    L = dict(zip(LAYOUT_NAMES, (int(v) for v in lay)))
    return ih[:L["BYTES"]].copy(), ig[:L["BYTES"]].copy(), L


def library_range(units, prm):
    """(bound, verdict) of the host-only entry point"""
    from rnnwavefunctions_amd import _lib
    lib = _lib.load_library()
    flat = flat_params(prm)
    bound, word = C.c_double(0.0), C.c_int32(-1)
    rc = lib.rnnwf_host_split_range(units, flat.ctypes.data_as(C.POINTER(C.c_double)), flat.size, C.byref(bound), C.byref(word))
    assert rc == 0, lib.rnnwf_last_error(None).decode()
    return bound.value, word.value


def range_word(img_g, L):
    return int(img_g[L["OFF_BD"] + 4 * RANGE_SLOT:L["OFF_BD"] + 4 * RANGE_SLOT + 4].view(np.uint32)[0])


def _bf16(a):
    return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def decode(img, L):
    """W[T, r32, hhk, e] float64 (row r32 of tile T, K entry e of lane half hhk), CI[sigma, T, r32], XC[sigma, hh, e]"""
    NT, NQ, NUP = L["NT"], L["NQ"], L["NUP"]
    assert 8 * NQ + 1 == NU and NT == 3 * NF32 + 2
    A = _bf16(img[:L["OFF_ASP"]].view(np.uint16).reshape(NT, 3, NQ, 64, 8))
    SP = _bf16(img[L["OFF_ASP"]:L["OFF_CI"]].view(np.uint16).reshape(NT, 64, 8))
    W = np.zeros((NT, 32, 2, NU))
    for hhk in range(2):
        lanes = slice(32 * hhk, 32 * hhk + 32)
        W[:, :, hhk, :NU - 1] = A[:, :, :, lanes, :].sum(axis=1).transpose(0, 2, 1, 3).reshape(NT, 32, 8 * NQ)
        W[:, :, hhk, NU - 1] = SP[:, lanes, 0] + SP[:, lanes, 3] + SP[:, lanes, 5]
    ci = img[L["OFF_CI"]:L["OFF_XC"]].view(np.float32).astype(np.float64).reshape(2, NT, 2, 16)
    r32 = np.arange(32)
    CI = ci[:, :, (r32 >> 2) & 1, (r32 & 3) + 4 * (r32 >> 3)]
    XC = img[L["OFF_XC"]:L["OFF_WD"]].view(np.float32).astype(np.float64).reshape(2, 2, NUP)[:, :, :NU]
    return W, CI, XC


def row_of(gate, e, hh):
    """(tile, row of the tile) of gate 0 r / 1 u / 2 q of the unit at entry e of lane half hh"""
    if e < 16 * NF32:
        T, rho = 3 * (e // 16) + gate, e % 16
    else:
        slot = gate * RJ + (e - 16 * NF32)
        T, rho = 3 * NF32 + slot // 16, slot % 16
    return T, (rho & 3) + 4 * hh + 8 * (rho >> 2)


def gate_rows(W, CI):
    """Wg[gate, hh, e, hhk, k], Cg[gate, sigma, hh, e]: the rows of every owned unit"""
    Wg = np.zeros((3, 2, NU, 2, NU))
    Cg = np.zeros((3, 2, 2, NU))
    for gate in range(3):
        for hh in range(2):
            for e in range(NU):
                T, r = row_of(gate, e, hh)
                Wg[gate, hh, e] = W[T, r]
                Cg[gate, :, hh, e] = CI[:, T, r]
    return Wg, Cg


def bounds(img_h, L):
    """A_u[hh, e], A_c[hh, e] from the image in h, float64"""
    W, CI, XC = decode(img_h, L)
    Wg, Cg = gate_rows(W, CI)
    rowsum = np.abs(Wg).sum(axis=(3, 4))
    A_u = np.abs(Cg[1]).max(axis=0) + rowsum[1]
    A_c = np.abs(XC).max(axis=0) + np.abs(Cg[2]).max(axis=0) + rowsum[2]
    return A_u, A_c


# ---- one gate tail on arrays: exact, the kernel's two forms in float32 -------------------------------------------------------------

def exact64(a_u, a_c, g):
    a_u, a_c, g = (np.asarray(x, dtype=np.float64) for x in (a_u, a_c, g))
    u, t = 1.0 / (1.0 + np.exp2(a_u)), 1.0 / (1.0 + np.exp2(a_c))
    return t + u * (g - t)


def _rcp32(x):
    """v_rcp_f32 as the worst case has it: a result below the normal range is flushed to zero"""
    with np.errstate(divide="ignore", over="ignore"):
        r = (np.float32(1.0) / x).astype(np.float32)
    return np.where(np.abs(r) < np.float32(2.0 ** -126), np.float32(0.0), r)


def two_rcp32(a_u, a_c, g):
    a_u, a_c, g = (np.asarray(x, dtype=np.float32) for x in (a_u, a_c, g))
    with np.errstate(over="ignore"):
        u = _rcp32(np.float32(1.0) + np.exp2(a_u))
        t = _rcp32(np.float32(1.0) + np.exp2(a_c))
    return (u * (g - t) + t).astype(np.float32)


def merged32(a_u, a_c, g):
    """(g', D): the merged sequence stage by stage, every operation rounded to float32 (the two fma of the kernel as fma: exact
    product, one rounding - float64 holds the product of two float32 exactly, the sum is rounded twice, within half an ulp more)"""
    a_u, a_c, g = (np.asarray(x, dtype=np.float32) for x in (a_u, a_c, g))
    with np.errstate(over="ignore", invalid="ignore"):
        Eu, Ec = np.exp2(a_u), np.exp2(a_c)
        D2 = (np.float32(1.0) + Ec).astype(np.float32)
        num = (g.astype(np.float64) * D2 + Eu).astype(np.float32)
        D = (Eu.astype(np.float64) * D2 + D2).astype(np.float32)
        return (num * _rcp32(D)).astype(np.float32), D
