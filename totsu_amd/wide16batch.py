"""`Wide16BatchSolver`: the wide batch (`WideBatchSolver`: many conic programs of one shape and cone layout, each with its OWN dense
A, of EVERY shape up to 4096 x 4096 and every PSD order up to 64, one workgroup per problem, all but the pass vectors left in the
problem's block of the arena) over a LIBRARY-OWNED 16-BIT COPY of every problem's A (thip_wide16batch_* in include/totsu_f32hip.h):
half the bytes of A per pass and half the memory, on the shapes where A is what a pass and a card's capacity are made of.  The
shapes, the cones (PSD included), the methods and the ValueErrors are `WideBatchSolver`'s; the store, a_dtype ("bf16" / "f16"),
`stored_a`, `widened` and the calls that convert are `Mid16BatchSolver`'s (totsu_amd/store16.py).

The problem solved is the one with the ROUNDED matrix W (`widened(i)`), and the batch is bit for bit a `WideBatchSolver` over W: the
whole arena block, the status blocks, `solutions()`, the preconditioner, at both workgroup sizes, in both state arithmetics, however
the iterations are cut into launches.  Its end iterate (`raw_iterate`) is a start (`set_iterates`) for a `WideBatchSolver` over the
exact matrix -- the batch form of the single solver's mixed route.

The f32 matrices are converted on the device at construction, by `replace`, `set_a` and `set_a_dev(values)`, and are not kept:
`set_a_dev(None)`, the in-place form, is refused.  No chooser returns this class: rounding the caller's matrix is never an automatic
choice."""
from . import _lib
from .store16 import Store16, kind_of, store_bytes_of
from .widebatch import WideBatchSolver


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_wide16batch_fits, which is the wide batch's; needs no GPU): (lds_bytes, threads), or ValueError"""
    from .ownbatch import _fits
    return _fits("thip_wide16batch_", n, m, seg_type, seg_len)


def _kind(a_dtype):
    return kind_of(a_dtype, "Wide16BatchSolver", "WideBatchSolver")


def store_bytes(n, m, a_dtype="f16"):
    """the bytes of one problem's block of the store (thip_wide16batch_store_bytes; needs no GPU)"""
    return store_bytes_of("thip_wide16batch_", n, m, _kind(a_dtype))


class Wide16BatchSolver(Store16, WideBatchSolver):
    """OwnBatchSolver on thip_wide16batch_*, with the additions of a family over a 16-bit store.  info() reports WideBatchSolver's
    fields (lds_bytes_per_problem, arena_bytes_per_problem, max_psd_order, n_psd, psd_lds_bytes) and a_dtype ("bf16" / "f16"),
    load_bytes (8), a_bytes_per_iter (bytes of the store read per problem-iteration), a_store_bytes."""
    _prefix, _force_hook, _what, _Info = "thip_wide16batch_", "thip_test_wide16batch_force_threads", "wide16", _lib.Wide16BatchInfo
    _name16, _name32 = "Wide16BatchSolver", "WideBatchSolver"
