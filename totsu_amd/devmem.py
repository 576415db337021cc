"""Device memory that is not the package's own: what the `_dev` methods of the own-A batches (totsu_amd/ownbatch.py) take and return.
`as_device(obj, what)` gives the address and the length of a float32 array on the GPU held as a `DeviceBuffer`, a torch tensor on
the GPU, or any object with `__cuda_array_interface__` (the protocol torch, cupy and numba speak on ROCm too); `offsets` is the one
rule of where each problem's part begins in a packed array.  Needs no GPU and imports no torch."""
import numpy as np

_TYPESTR = {"<f4": "float32", "<i4": "int32"}


def is_torch(obj):
    """a torch tensor, told by its type's module: torch is not imported for the question"""
    return type(obj).__module__.split(".")[0] == "torch" and hasattr(obj, "data_ptr")


def _contiguous(shape, strides, itemsize):
    """C-contiguous by the interface's rule: strides None, or those of a packed row-major array (an axis of length 1 may say anything)"""
    if strides is None:
        return True
    want = itemsize
    for n, s in zip(reversed(tuple(shape)), reversed(tuple(strides))):
        if n != 1 and s != want:
            return False
        want *= n
    return True


def as_device(obj, what, out=False, typestr="<f4"):
    """(address, number of elements) of the device array `obj`: a DeviceBuffer, a torch tensor on the GPU, or an object with
    __cuda_array_interface__.  ValueError, with `what` in the message: another dtype than float32 (typestr: "<i4" for a state
    array), strides that are not those of a packed array, a tensor on the host, a read-only array where an output is wanted (out)."""
    from .fused import DeviceBuffer
    name = _TYPESTR[typestr]
    if isinstance(obj, DeviceBuffer):
        if obj.ptr is None:
            raise ValueError("%s: the DeviceBuffer has been freed" % what)
        return int(obj.ptr), int(obj.n)         # (a DeviceBuffer is 4-byte words: it serves as float32 and as int32)
    if is_torch(obj):
        if not obj.is_cuda:
            raise ValueError("%s: a tensor on the host (device %s) where device memory is needed" % (what, obj.device))
        if str(obj.dtype) != "torch." + name:
            raise ValueError("%s: dtype %s where %s is needed" % (what, obj.dtype, name))
        if not obj.is_contiguous():
            raise ValueError("%s: the tensor is not contiguous (strides %r)" % (what, tuple(obj.stride())))
        return int(obj.data_ptr()), int(obj.numel())
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        if isinstance(obj, np.ndarray) or hasattr(obj, "__array_interface__"):
            raise ValueError("%s: an array on the host where device memory is needed" % what)
        raise ValueError("%s: a DeviceBuffer, a torch tensor on the GPU or an object with __cuda_array_interface__ is needed, not %s"
                         % (what, type(obj).__name__))
    if cai.get("typestr") != typestr:
        raise ValueError("%s: dtype %r where %s (%r) is needed" % (what, cai.get("typestr"), name, typestr))
    shape = tuple(int(v) for v in cai["shape"])
    if not _contiguous(shape, cai.get("strides"), 4):
        raise ValueError("%s: the array is not contiguous (shape %r, strides %r)" % (what, shape, tuple(cai["strides"])))
    ptr, readonly = cai["data"]
    if out and readonly:
        raise ValueError("%s: a read-only array where an output is wanted" % what)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if n and not ptr:
        raise ValueError("%s: a null address" % what)
    return int(ptr or 0), n


def offsets(lengths):
    """where each part begins in a packed array whose parts have the given lengths, and (the last entry) the array's length"""
    at = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=at[1:])
    return at


def part_lengths(n, m):
    """the lengths of one problem's part in the packed arrays of the `_dev` calls, in the order thip_test_ownbatch_offsets reports
    them: c / a solution's x, b / row sums / a solution's y, an iterate's x, its y, a dense A"""
    n, m = int(n), int(m)
    return n, m, n + 2 * m + 1, n + m + 1, m * n
