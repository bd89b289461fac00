"""Specification of the split weight packs in plain numpy (tests/test_host_split_table.py on the CPU, tests/test_gpu_split_packs.py
on the GPU).  No library call and no GPU: a step of the table (mtadgat_split_steps, include/mtadgat.h) is replayed on a float32 copy
of the packed image, from the layout comments of csrc/mtadgat_device.h, csrc/mtadgat_host.h and csrc/mtadgat_packdev.hip.

Words.  The image is addressed in floats.  A word is 64 lanes x 16 bytes = 256 floats.  An fp32 pack is [outer][Qs chunks][G gates]
words of 4 floats per lane.  A 16-bit pack is [outer][Qd chunks][G][pieces] words of 8 elements per lane, little endian: elements 0-3
of a lane are its four floats of source chunk 2 qd, elements 4-7 those of chunk 2 qd + 1; a chunk index >= Qs reads as zeros.

Pieces.  Three bf16 pieces: hi = bf16(v), mid = bf16(v - hi), lo = bf16((v - hi) - mid), float32 subtractions, round to nearest
even.  Two fp16 pieces of S v: hi = f16(S v), lo = f16(S v - hi).  S is the power of two that puts the group's largest |weight| into
[2^13, 2^14); the slot of a group is [bits of the maximum, S, 1 / S, 0]."""
import numpy as np

WORD = 256                      # floats per word
OPS = ("ZERO_SCALE", "ABSMAX", "SCALE_FROM_MAX", "SPLIT3", "SPLIT2H", "SPLIT2H_GATH", "SPLIT_X", "REORDER_XQ")
SCALE_OPS = OPS[:3]
SPLIT_OPS = ("SPLIT3", "SPLIT2H", "SPLIT2H_GATH", "SPLIT_X")


# ---- conversions ----------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even on the uint32 view."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f16_to_f32(h):
    return np.asarray(h, dtype=np.uint16).view(np.float16).astype(np.float32)


def split3(v):
    """(hi, mid, lo) bf16 bit patterns of a float32 array."""
    v = np.asarray(v, dtype=np.float32)
    hi = bf16_rne(v)
    r = v - bf16_to_f32(hi)
    mid = bf16_rne(r)
    s = r - bf16_to_f32(mid)
    return hi, mid, bf16_rne(s)


def split2h(v):
    """(hi, lo) fp16 bit patterns of a float32 array (already scaled)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def scale_slot(max_bits):
    """[bits, S, 1 / S, 0] as four uint32 for the bits of the largest |value|: S = 2^(14 - e) with max = f 2^e, f in [0.5, 1), the
    exponent clamped to +-100; e = 0 for a zero, infinite or >= 3e38 maximum."""
    m = np.array([max_bits], dtype=np.uint32).view(np.float32)[0]
    e = 0
    if m > 0 and m < np.float32(3.0e38):
        e = int(np.frexp(m)[1])
    sh = max(-100, min(100, 14 - e))
    f = np.array([np.ldexp(np.float32(1), sh), np.ldexp(np.float32(1), -sh), 0.0], dtype=np.float32)
    return np.concatenate([np.array([max_bits], dtype=np.uint32), f.view(np.uint32)])


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def _round_up(n, m):
    return (n + m - 1) // m * m


def pair_chunks(src, outer, Qs, Qd, G):
    """fp32 pack [outer][Qs][G][64][4] -> the element order of its 16-bit pack, (outer, Qd, G, 64, 8) float32."""
    a = np.asarray(src, dtype=np.float32).reshape(outer, Qs, G, 64, 4)
    keep = min(Qs, 2 * Qd)                                          # (2 Qd < Qs would drop chunks: the table test forbids it)
    p = np.zeros((outer, 2 * Qd, G, 64, 4), dtype=np.float32)
    p[:, :keep] = a[:, :keep]
    p = p.reshape(outer, Qd, 2, G, 64, 4)
    return np.ascontiguousarray(np.moveaxis(p, 2, 4)).reshape(outer, Qd, G, 64, 8)


def _words(pieces):
    """piece arrays (..., 64, 8) uint16 -> (..., pieces, 64, 8) uint16"""
    return np.stack(pieces, axis=-3)


def _as_f32(u16):
    return np.ascontiguousarray(u16).reshape(-1).view(np.float32)


def compact_columns(ncols, E, P8, PT, npos):
    """k_gath's compact column order as a list: source column (of the 8-padded fp32 pack) of every destination column, -1 = zeros."""
    nneg = E - npos
    P2 = _round_up(npos, 2)
    PT2 = _round_up(P2 + nneg, 8)
    cols = list(range(npos))
    cols += [-1] * (P2 - npos)
    cols += [P8 + i for i in range(nneg)]
    cols += [-1] * (PT2 - len(cols))
    cols += [PT]                                                    # the c / d column
    cols += [-1] * (ncols - len(cols))
    assert len(cols) == ncols, (ncols, E, P8, PT, npos)
    return cols


# ---- footprints -----------------------------------------------------------------------------------------------------------------
def x_words(step):
    """words per outer block of a SPLIT_X destination"""
    return step["arg"] * 9 + (step["Qd"] - step["arg"]) * 6


def footprint(step):
    """(src floats, dst floats) a step reads (from step["src"]) and writes (at step["dst"]; the scale ops: at step["scale"])."""
    op, n, Qs, Qd, arg = step["op"], step["n"], step["Qs"], step["Qd"], step["arg"]
    if op == "ZERO_SCALE":
        return 0, 4
    if op == "ABSMAX":
        return n, 1
    if op == "SCALE_FROM_MAX":
        return 0, 4
    if op == "SPLIT3":
        return n * Qs * WORD, n * Qd * 3 * WORD
    if op == "SPLIT2H":
        return n * Qs * arg * WORD, n * Qd * arg * 2 * WORD
    if op == "SPLIT2H_GATH":
        return 2 * n * Qs * WORD, 2 * n * Qd * 2 * WORD
    if op == "SPLIT_X":
        return n * Qs * 3 * WORD, n * x_words(step) * WORD
    if op == "REORDER_XQ":
        return n * Qd * 6 * WORD, n * Qd * 6 * WORD
    raise ValueError(op)


def dst_span(step):
    """(offset, floats) written"""
    return (step["scale"] if step["op"] in SCALE_OPS else step["dst"]), footprint(step)[1]


def locate(step, i):
    """Where float i of a step's destination sits: dict of outer, chunk, gate, piece, lane, element (the first of the two 16-bit
    elements of the float); the scale ops: the index within the slot."""
    op, Qd = step["op"], step["Qd"]
    if op in SCALE_OPS:
        return dict(slot=i)
    w, r = divmod(i, WORD)
    lane, el = r // 4, 2 * (r % 4)
    if op in ("SPLIT3", "SPLIT2H", "SPLIT2H_GATH"):
        P = 3 if op == "SPLIT3" else 2
        G = step["arg"] if op == "SPLIT2H" else 1
        w, piece = divmod(w, P)
        w, gate = divmod(w, G)
        outer, chunk = divmod(w, Qd)
    elif op == "SPLIT_X":
        qb = step["arg"]
        outer, w = divmod(w, x_words(step))
        if w < 9 * qb:
            chunk, w = divmod(w, 9)
            gate, piece = divmod(w, 3)
        else:
            chunk, w = divmod(w - 9 * qb, 6)
            chunk += qb
            gate, piece = divmod(w, 2)
    else:                                                           # REORDER_XQ: [chunk][tile][gate][piece]
        w, k = divmod(w, 6)
        chunk, outer = divmod(w, step["n"])
        gate, piece = divmod(k, 2)
    return dict(outer=outer, chunk=chunk, gate=gate, piece=piece, lane=lane, element=el)


# ---- one function per op: each replays a step on the image (float32 array) in place ---------------------------------------------
def _u32(img):
    return img.view(np.uint32)


def _S(img, step):
    return img[step["scale"] + 1]


def op_zero_scale(img, step):
    _u32(img)[step["scale"]:step["scale"] + 4] = 0


def op_absmax(img, step):
    src = img[step["src"]:step["src"] + step["n"]]
    m = np.abs(src).max() if src.size else np.float32(0)
    bits = np.array([m], dtype=np.float32).view(np.uint32)[0]       # non-negative floats order like unsigned integers
    u = _u32(img)
    u[step["scale"]] = max(u[step["scale"]], bits)


def op_scale_from_max(img, step):
    u = _u32(img)
    u[step["scale"]:step["scale"] + 4] = scale_slot(u[step["scale"]])


def _src(img, step):
    return img[step["src"]:step["src"] + footprint(step)[0]]


def _store(img, step, f32):
    assert f32.size == footprint(step)[1], (step, f32.size)
    img[step["dst"]:step["dst"] + f32.size] = f32


def op_split3(img, step):
    v = pair_chunks(_src(img, step), step["n"], step["Qs"], step["Qd"], 1)
    _store(img, step, _as_f32(_words(split3(v))))


def op_split2h(img, step):
    v = pair_chunks(_src(img, step), step["n"], step["Qs"], step["Qd"], step["arg"]) * _S(img, step)
    _store(img, step, _as_f32(_words(split2h(v))))


def gath_gather(v, NT_L, cols):
    """(2, NT_L, Qd, 64, 8) in the fp32 pack's column order -> the same in the order `cols`.  Column c of tile n is lane c & 31 of
    both 32-lane halves (the halves hold different features of the same column)."""
    Qd = v.shape[2]
    bycol = v.reshape(2, NT_L, Qd, 2, 32, 8).transpose(0, 2, 3, 1, 4, 5).reshape(2, Qd, 2, NT_L * 32, 8)
    out = np.zeros_like(bycol)
    for c, cs in enumerate(cols):
        if cs >= 0:
            out[:, :, :, c] = bycol[:, :, :, cs]
    return np.ascontiguousarray(out.reshape(2, Qd, 2, NT_L, 32, 8).transpose(0, 3, 1, 2, 4, 5)).reshape(2, NT_L, Qd, 64, 8)


def op_split2h_gath(img, step):
    NT_L, Qd = step["n"], step["Qd"]
    P8, PT, npos = (int(x) for x in img.view(np.int32)[step["ord"]:step["ord"] + 3])
    cols = compact_columns(32 * NT_L, step["arg"], P8, PT, npos)
    v = pair_chunks(_src(img, step), 2 * NT_L, step["Qs"], Qd, 1).reshape(2, NT_L, Qd, 64, 8)
    v = gath_gather(v, NT_L, cols).reshape(2 * NT_L, Qd, 1, 64, 8) * _S(img, step)
    _store(img, step, _as_f32(_words(split2h(v))))


def op_split_x(img, step):
    n, Qd, qb = step["n"], step["Qd"], step["arg"]
    v = pair_chunks(_src(img, step), n, step["Qs"], Qd, 3) * _S(img, step)
    head = _words(split3(v[:, :qb])).reshape(n, -1)                 # chunks below qb: [gate][3 bf16 pieces], 9 words
    tail = _words(split2h(v[:, qb:])).reshape(n, -1)                # the rest: [gate][2 fp16 pieces], 6 words
    _store(img, step, _as_f32(np.concatenate([head, tail], axis=1)))


def op_reorder_xq(img, step):
    n, Qd = step["n"], step["Qd"]
    src = _src(img, step).reshape(n, Qd, 6 * WORD)                  # [tile][chunk][6 words] -> [chunk][tile][6 words]
    _store(img, step, np.ascontiguousarray(src.transpose(1, 0, 2)).reshape(-1))


REPLAY = dict(ZERO_SCALE=op_zero_scale, ABSMAX=op_absmax, SCALE_FROM_MAX=op_scale_from_max, SPLIT3=op_split3, SPLIT2H=op_split2h,
              SPLIT2H_GATH=op_split2h_gath, SPLIT_X=op_split_x, REORDER_XQ=op_reorder_xq)


def replay(image, steps):
    """A copy of the image (float32 array) with every step applied in order."""
    img = np.array(image, dtype=np.float32, copy=True)
    for s in steps:
        REPLAY[s["op"]](img, s)
    return img


# ---- decoding a device pack (the contract checks, independent of the replay) ----------------------------------------------------
def decode(img, step):
    """The 16-bit pieces a split step wrote, against the values they stand for: a list of dicts
        kind    "bf16" (three pieces) or "f16" (two)
        sv      S v as float32, (..., 64, 8), recomputed from the image's own fp32 source and scale slot (S = 1 for SPLIT3)
        bits    the pieces as stored, uint16 (P, ..., 64, 8)
        pieces  their values as float64
        pad     True where the layout reads zeros instead of a source value: chunks >= Qs, and for SPLIT2H_GATH the padding columns
                of the compact order (taken from the image's own ord)"""
    op, n, Qs, Qd, arg = step["op"], step["n"], step["Qs"], step["Qd"], step["arg"]
    d16 = np.ascontiguousarray(img[step["dst"]:step["dst"] + footprint(step)[1]]).view(np.uint16)
    src = _src(img, step)
    G = {"SPLIT3": 1, "SPLIT2H": arg, "SPLIT2H_GATH": 1, "SPLIT_X": 3}[op]
    outer = 2 * n if op == "SPLIT2H_GATH" else n
    v = pair_chunks(src, outer, Qs, Qd, G)
    real = pair_chunks(np.ones_like(src), outer, Qs, Qd, G)
    if op == "SPLIT2H_GATH":
        P8, PT, npos = (int(x) for x in img.view(np.int32)[step["ord"]:step["ord"] + 3])
        cols = compact_columns(32 * n, arg, P8, PT, npos)
        v, real = (gath_gather(a.reshape(2, n, Qd, 64, 8), n, cols).reshape(outer, Qd, 1, 64, 8) for a in (v, real))
    if op != "SPLIT3":
        v = v * _S(img, step)
    pad = real == 0

    def part(kind, sv, pd, u16):                                    # u16: (..., P, 64, 8)
        conv = bf16_to_f32 if kind == "bf16" else f16_to_f32
        bits = np.moveaxis(u16, -3, 0)
        return dict(kind=kind, sv=sv, pad=pd, bits=bits, pieces=conv(np.ascontiguousarray(bits)).astype(np.float64))

    if op == "SPLIT3":
        return [part("bf16", v, pad, d16.reshape(n, Qd, 1, 3, 64, 8))]
    if op in ("SPLIT2H", "SPLIT2H_GATH"):
        return [part("f16", v, pad, d16.reshape(outer, Qd, G, 2, 64, 8))]
    if op == "SPLIT_X":
        d = d16.reshape(n, -1)
        nh = arg * 9 * 512
        return [part("bf16", v[:, :arg], pad[:, :arg], d[:, :nh].reshape(n, arg, 3, 3, 64, 8)),
                part("f16", v[:, arg:], pad[:, arg:], d[:, nh:].reshape(n, Qd - arg, 3, 2, 64, 8))]
    raise ValueError(op)


def f16_bound(sv):
    """the two-fp16-piece contract of csrc/mtadgat_device.h: |S v - hi - lo| <= max(2^-22 |S v|, 2^-25)"""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(sv, dtype=np.float64)), 2.0 ** -25)


def check_contract(img, steps, what=""):
    """Independent of the replay: the pieces as stored in the image against the image's own fp32 source and scale slot.  Three bf16
    pieces sum to S v exactly, two fp16 pieces to within f16_bound, and padding is all-zero bits."""
    for k, s in enumerate(steps):
        if s["op"] not in SPLIT_OPS:
            continue
        for part in decode(img, s):
            if part["sv"].size == 0:
                continue
            sv = part["sv"].astype(np.float64)
            got = part["pieces"].sum(axis=0)
            if part["kind"] == "bf16":
                assert np.array_equal(got, sv), (what, k, s["op"], "three bf16 pieces do not sum to the value", float(np.abs(got - sv).max()))
            else:
                err, bound = np.abs(sv - got), f16_bound(sv)
                assert np.all(err <= bound), (what, k, s["op"], "two fp16 pieces miss max(2^-22 |S v|, 2^-25): worst error / bound",
                                              float((err / bound).max()))
                assert np.abs(sv).max() < 2.0 ** 14, (what, k, s["op"], float(np.abs(sv).max()))
            assert not part["bits"][:, part["pad"]].any(), (what, k, s["op"], "padding is not all-zero bits")
