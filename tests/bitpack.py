"""MSB-first bit packer for hand-written known-answer packets (tests only)."""


def pack(fields, slack=0):
    """fields: iterable of (nbits, value) or a '0101' string.  Zero-padded to a byte + `slack` bytes."""
    parts = []
    for f in fields:
        if isinstance(f, str):
            parts.append("".join(c for c in f if c in "01"))
        else:
            nbits, value = f
            if nbits > 0:
                parts.append(format(value & ((1 << nbits) - 1), "0%db" % nbits))
    bits = "".join(parts)
    bits += "0" * (-len(bits) % 8)
    out = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return out + bytes(slack)
