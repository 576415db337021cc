"""`Mid16BatchSolver`: the mid batch (`MidBatchSolver`: many mid-size conic programs of one shape and cone layout, each with its OWN
dense A streamed by one workgroup per problem) over a LIBRARY-OWNED 16-BIT COPY of every problem's A (thip_mid16batch_* in
include/totsu_f32hip.h): half the bytes of A per pass, half the memory, and one load path for every m (the store pads the leading
dimension).  The shapes, the cones, the methods and the ValueErrors are `MidBatchSolver`'s.

a_dtype, fixed at construction: "bf16" -- the f32 rounded to nearest even to its upper 16 bits -- or "f16" -- one power-of-two scale
per column, inv_s[c] = 2^(e - 14) with e the exponent frexp gives the column's largest |a| (1 for a column of zeros), and the word
f16(a / inv_s[c]).  The problem solved is the one with the ROUNDED matrix W (`widened(i)`): W(r, c) the bf16 word shifted left 16
bits, or float32(h(r, c)) * inv_s[c].  The batch is bit for bit a `MidBatchSolver` over W.  Its end iterate (`raw_iterate`) is a
start (`set_iterates`) for a `MidBatchSolver` over the exact matrix -- the batch form of the single solver's mixed route.

The f32 matrices are converted on the device at construction, by `replace`, `set_a` and `set_a_dev(values)`, and are not kept:
`set_a_dev(None)`, the in-place form, is refused.  No chooser returns this class: rounding the caller's matrix is never an automatic
choice."""
from . import _lib
from .midbatch import MidBatchSolver
from .store16 import Store16, kind_of, store_bytes_of


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_mid16batch_fits, which is the mid batch's; needs no GPU): (lds_bytes, threads), or ValueError"""
    from .ownbatch import _fits
    return _fits("thip_mid16batch_", n, m, seg_type, seg_len)


def _kind(a_dtype):
    return kind_of(a_dtype, "Mid16BatchSolver", "MidBatchSolver")


def store_bytes(n, m, a_dtype="f16"):
    """the bytes of one problem's block of the store (thip_mid16batch_store_bytes; needs no GPU)"""
    return store_bytes_of("thip_mid16batch_", n, m, _kind(a_dtype))


class Mid16BatchSolver(Store16, MidBatchSolver):
    """OwnBatchSolver on thip_mid16batch_*, with the additions of a family over a 16-bit store (totsu_amd/store16.py: a_dtype,
    replace / set_a_dev on the store, stored_a, widened).  info() reports a_dtype ("bf16" / "f16"), load_bytes (8), a_bytes_per_iter
    (bytes of the store read per problem-iteration) and a_store_bytes."""
    _prefix, _force_hook, _what, _Info = "thip_mid16batch_", "thip_test_mid16batch_force_threads", "mid16", _lib.Mid16BatchInfo
    _name16, _name32 = "Mid16BatchSolver", "MidBatchSolver"
