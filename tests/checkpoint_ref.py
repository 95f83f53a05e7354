"""Host reference of the checkpoint digest (include/cadre_hip.h, cadre_state_capture), independent of the package:

    D = sum_i (uint64(w_i) + 1) * ((2 i + 1) * 0x9E3779B97F4A7C15)   mod 2^64

over the 32-bit words of a range.  numpy uint64 ARRAY arithmetic wraps silently, which is the definition."""
import numpy as np

K = np.uint64(0x9E3779B97F4A7C15)

# bit patterns every operand set carries: +0, -0.0, quiet / signalling NaNs with payloads, infinities, all ones, 1
SPECIAL = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000,
                    0xFFFFFFFF, 0x00000001], dtype=np.uint32)


def terms(words):
    """The summands, one uint64 per 32-bit word."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    m = (np.uint64(2) * i + np.uint64(1)) * K
    return (w + np.uint64(1)) * m


def digest(words):
    return int(terms(words).sum(dtype=np.uint64))


def as_i64(d):
    """The uint64 digest as the int64 bit pattern the device tensors hold."""
    return int(np.array([d], dtype=np.uint64).view(np.int64)[0])


def random_words(r, n):
    """n random 32-bit patterns with the SPECIAL ones sprinkled in (first and last word included when there is room)."""
    w = r.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        k = min(n, len(SPECIAL))
        pos = r.permutation(n)[:k]
        w[pos] = SPECIAL[r.permutation(len(SPECIAL))[:k]]
    return w
