"""COCO compressed run-length strings, restated sequentially: one value, one character at a time, written from the description
of the coding in include/gigapose_rlestr.h.  The independent reference of the tests for the vectorised host codec
(gigapose_amd/rle_strings.py) and for the kernel (libgigapose_rlestr.so); deliberately shares no code with either.

  list position m carries x = counts[m] (m <= 2) or counts[m] - counts[m-2] (m >= 3);
  x is written as little-endian 5-bit groups, one per character c + 48; bit 0x20 of c: another group follows; bit 0x10 of the
  last group: the sign."""
import numpy as np


def encode_value(x):
    """One (possibly negative) integer -> its characters."""
    x = int(x)
    out = []
    more = True
    while more:
        c = x & 0x1f
        x >>= 5                                            # Python's >> on an int is arithmetic
        more = (x != -1) if (c & 0x10) else (x != 0)
        if more:
            c |= 0x20
        out.append(c + 48)
    return bytes(out)


def encode_counts(counts):
    counts = [int(c) for c in counts]
    return b"".join(encode_value(c - counts[m - 2] if m >= 3 else c) for m, c in enumerate(counts))


def decode_values(s):
    """The string -> the list of x, one per token.  Raises ValueError on a character outside 48 .. 111, on a token of more than 7
    characters and on a string that stops inside a token."""
    if isinstance(s, str):
        s = s.encode("ascii")
    xs, x, k = [], 0, 0
    for pos, ch in enumerate(s):
        if not 48 <= ch <= 111:
            raise ValueError(f"character {ch} at {pos} is outside 48 .. 111")
        c = ch - 48
        x |= (c & 0x1f) << (5 * k)
        k += 1
        if k > 7:
            raise ValueError(f"the token that holds character {pos} is longer than 7 characters")
        if not c & 0x20:
            if c & 0x10:
                x -= 1 << (5 * k)                          # sign extension from bit 5k (k groups read)
            xs.append(x)
            x, k = 0, 0
    if k:
        raise ValueError("the string stops inside a token")
    return xs


def decode_counts(s):
    counts = []
    for m, x in enumerate(decode_values(s)):
        counts.append(x + counts[m - 2] if m >= 3 else x)
    return np.asarray(counts, np.int64)
