"""A model of what k_rbsp must compute, from the clause text.

H.265 7.3.1.1: nal_unit() copies rbsp bytes until it meets next_bits(24) ==
0x000003, where it copies two bytes and skips the third, the
emulation_prevention_three_byte; 7.4.2 says that byte follows 0x0000 where the
payload would otherwise hold 0x000000 .. 0x000003 there, or where the payload's
last byte is 0x00 (cabac_zero_words end in 0x0000 03).  The reference scans the
same way (src/hevc/rbsp_reader.rs:11-39): at a zero byte followed by 00 03 it
keeps the two zeros and skips the 03 when the byte after it is <= 3 or the 03
ends the payload, and resumes behind the 03; anywhere else it moves on by one
byte.  unescape() below is that scan, one state variable and no look-behind
into the input.

7.4.7.1: the slice header's entry points count bytes of the slice segment data
WITH its emulation prevention bytes.  A substream-table entry e (raw offset in
the low 30 bits, SUB_* flags above) therefore becomes min(e, len) minus the
removed bytes at positions below it, with the flags as they were; an entry at
or past the payload's end becomes the RBSP length.
"""
SUB_OFFSET = 0x3fffffff
SUB_CONTINUE = 1 << 30
SUB_SEG_END = 1 << 31


def unescape(raw):
    """(rbsp bytes, ascending raw positions of the removed bytes)"""
    raw = bytes(raw)
    out, removed = bytearray(), []
    zeros = 0  # zero bytes copied out in a row, before raw[i]
    i, n = 0, len(raw)
    while i < n:
        b = raw[i]
        if zeros >= 2 and b == 3 and (i + 1 == n or raw[i + 1] <= 3):
            removed.append(i)
            zeros = 0
        else:
            out.append(b)
            zeros = zeros + 1 if b == 0 else 0
        i += 1
    return bytes(out), removed


def remap(raw, entries):
    """The entries of one picture's substream table (every word k_rbsp remaps: the
    substream starts, the end entry, the segment starts inside rows) in RBSP offsets."""
    rbsp, removed = unescape(raw)
    out = []
    for w in entries:
        e, flags = min(w & SUB_OFFSET, len(raw)), w & ~SUB_OFFSET & 0xffffffff
        out.append((e - sum(1 for r in removed if r < e)) | flags)
    return rbsp, out


def predicate(raw):
    """kernels/rbsp.hip's header comment: position i is removed iff raw[i-2] == 0,
    raw[i-1] == 0, raw[i] == 3 and (i + 1 == len or raw[i+1] <= 3); the two bytes
    before the payload are not both zero."""
    n = len(raw)
    return [i for i in range(2, n) if raw[i] == 3 and raw[i - 1] == 0 and raw[i - 2] == 0
            and (i + 1 == n or raw[i + 1] <= 3)]
