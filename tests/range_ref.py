"""The statement of l2i_range_stats (include/l2i.h) in numpy, from RAW bit patterns: no float arithmetic decides a bin.

``row(bits, kind, into=None)`` returns the 260 words one call adds to ``into`` (zeros when absent):
  [0..255]  elements per biased fp32 exponent field of the value converted exactly to fp32 (0: zeros and fp32 subnormals; 255: inf / NaN),
  [256]     exact +-0,  [257] max over the finite elements of |x| as fp32 bits (unsigned),  [258] += 1,  [259] += n.
fp16 -> fp32 is done on integers: normals re-bias the exponent by 112 and shift the mantissa by 13; subnormals m * 2^-24 are normalised by the position of
m's top bit (fields 103 .. 112); bf16 is the top half of an fp32 pattern.

``MISTAKES`` are wrong versions of the same statement, each one slip an implementation can make; tests/test_range_ref_cpu.py shows that the
hand-made cases tell every one of them from ``row``."""
import numpy as np

F16, BF16, F32 = 0, 1, 2
WORDS, ZEROS, MAX, CALLS, N = 260, 256, 257, 258, 259
NP_BITS = {F16: np.uint16, BF16: np.uint16, F32: np.uint32}


def f16_abs_bits(h):
    """uint16 patterns -> uint32 patterns of |x| as fp32, exactly."""
    h = np.asarray(h).astype(np.uint32)
    e, m = (h >> 10) & 31, h & 0x3ff
    out = np.where(e == 31, np.uint32(0x7f800000) | (m << 13), ((e + 112) << 23) | (m << 13)).astype(np.uint32)
    top = np.zeros_like(m)                                       # floor(log2 m) for m >= 1, by comparison (integers only)
    for p in range(1, 10):
        top = np.where(m >= (1 << p), p, top)
    sub = ((top + 103) << 23) | ((m << (23 - top)) & 0x7fffff)
    return np.where(e == 0, np.where(m == 0, 0, sub), out).astype(np.uint32)


def abs_bits(bits, kind):
    if kind == F16:
        return f16_abs_bits(bits)
    if kind == BF16:
        return (np.asarray(bits).astype(np.uint32) & 0x7fff) << 16
    if kind == F32:
        return np.asarray(bits).astype(np.uint32) & 0x7fffffff
    raise ValueError('kind %r' % (kind,))


def row(bits, kind, into=None):
    a = abs_bits(np.asarray(bits).reshape(-1), kind)
    out = np.zeros(WORDS, dtype=np.uint64) if into is None else np.array(into, dtype=np.uint64)
    field = (a >> 23).astype(np.int64)
    out[:256] += np.bincount(field, minlength=256).astype(np.uint64)
    out[ZEROS] += np.uint64(int((a == 0).sum()))
    finite = a[field != 255]
    out[MAX] = max(int(out[MAX]), int(finite.max()) if finite.size else 0)
    out[CALLS] += np.uint64(1)
    out[N] += np.uint64(a.size)
    return out


# ---- planted mistakes: (name, function with row's signature) -----------------------------------------------------------------------------------------
def _max_over_inf(bits, kind, into=None):
    out = row(bits, kind, into)
    a = abs_bits(np.asarray(bits).reshape(-1), kind)
    out[MAX] = max(int(out[MAX]), int(a.max()))                  # inf / NaN patterns are the largest unsigned numbers there are
    return out


def _max_signed(bits, kind, into=None):
    out = row(bits, kind, None)
    b = np.asarray(bits).reshape(-1)
    if kind == F32:
        full = b.astype(np.uint32)
    elif kind == BF16:
        full = b.astype(np.uint32) << 16
    else:
        full = f16_abs_bits(b) | ((b.astype(np.uint32) >> 15) << 31)
    a = full & 0x7fffffff
    vals = full.view(np.int32)[(a >> 23) != 255]                 # compared as SIGNED numbers: every negative value loses to zero
    out[MAX] = max(int(vals.max()), 0) if vals.size else 0
    return _merge(out, into)


def _f16_subnormals_at_zero(bits, kind, into=None):
    out = row(bits, kind, None)
    if kind == F16:
        moved = int(out[103:113].sum())
        out[103:113] = 0
        out[0] += np.uint64(moved)                               # a flushing convert: the subnormals land in field 0 (and not among the zeros)
    return _merge(out, into)


def _bf16_as_f16(bits, kind, into=None):
    return row(bits, F16 if kind == BF16 else kind, into)


def _zeros_missing_from_field_0(bits, kind, into=None):
    out = row(bits, kind, None)
    out[0] -= out[ZEROS]
    return _merge(out, into)


def _overwrites(bits, kind, into=None):
    return row(bits, kind, None)


def _merge(one, into):
    if into is None:
        return one
    out = np.array(into, dtype=np.uint64)
    out[:257] += one[:257]
    out[MAX] = max(int(out[MAX]), int(one[MAX]))
    out[CALLS] += one[CALLS]
    out[N] += one[N]
    return out


MISTAKES = [('max taken over inf', _max_over_inf), ('max signed', _max_signed), ('fp16 subnormals binned at 0', _f16_subnormals_at_zero),
            ('bf16 read as fp16', _bf16_as_f16), ('zeros missing from field 0', _zeros_missing_from_field_0), ('overwrites instead of adding', _overwrites)]


# ---- hand-made cases: kind -> (bit patterns, {word: expected}) ------------------------------------------------------------------------------------------
def specials(kind):
    """The special values of a kind as raw patterns, with what every one of them must do to the row, written out by hand."""
    if kind == F16:
        #        +0      -0      min sub  max sub  min normal  largest finite (negative: -65504)  +inf    -inf    NaN payloads
        bits = [0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0xfbff, 0x7c00, 0xfc00, 0x7c01, 0xfe55, 0x3c00]
        want = {0: 2, ZEROS: 2, 103: 1, 112: 1, 113: 1, 142: 1, 255: 4, 127: 1, MAX: 0x477fe000, N: 11, CALLS: 1}       # 65504 = 0x477fe000
    elif kind == BF16:
        #        +0      -0      min sub  max sub  min normal  largest finite (negative)  +inf    -inf    NaN payloads     1.0
        bits = [0x0000, 0x8000, 0x0001, 0x007f, 0x0080, 0xff7f, 0x7f80, 0xff80, 0x7f81, 0xffd5, 0x3f80]
        want = {0: 4, ZEROS: 2, 1: 1, 254: 1, 255: 4, 127: 1, MAX: 0x7f7f0000, N: 11, CALLS: 1}
    else:
        bits = [0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xffc12345, 0x3f800000]
        want = {0: 4, ZEROS: 2, 1: 1, 254: 1, 255: 4, 127: 1, MAX: 0x7f7fffff, N: 11, CALLS: 1}
    return np.array(bits, dtype=NP_BITS[kind]), want
