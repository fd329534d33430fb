#!/usr/bin/env python3
"""Regenerates the 128-entry table of csrc/pft_cosh.h (the table of the published exp algorithm,
N = 128) from first principles, with mpmath at 200 bits:

    v = 2^(k/128),  H = double(v),  T = double(v / H - 1)          k = 0 .. 127
    entry k = { bits(T), bits(H) - (k << 45) }

so that 2^(k/128) ~ H (1 + T) and adding k << 45 (k's low 7 bits moved to the exponent's bottom)
to the second word of the entry ki % 128 gives the bits of 2^floor(ki/128) H.

    python scripts/gen_exp_table.py            prints the literals as they stand in pft_cosh.h
    python scripts/gen_exp_table.py --check    compares them with the header's, exit status 1 if
                                               they differ
"""
import os
import re
import struct
import sys

import mpmath

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "porousfreezethaw_amd", "csrc",
                      "pft_cosh.h")


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def table():
    mpmath.mp.prec = 200
    out = []
    for k in range(128):
        v = mpmath.power(2, mpmath.mpf(k) / 128)
        H = float(v)                       # mpmath rounds to nearest even
        T = float(v / mpmath.mpf(H) - 1)
        out.append((bits(T), (bits(H) - (k << 45)) & 0xFFFFFFFFFFFFFFFF))
    return out


def literals(tab):
    lines = []
    for k in range(0, 128, 2):
        lines.append("\t" + " ".join("{0x%016xULL, 0x%016xULL}," % e for e in tab[k:k + 2]) + " \\")
    lines[-1] = lines[-1][:-3]
    return "\n".join(lines)


def main():
    tab = table()
    if "--check" in sys.argv[1:]:
        text = open(HEADER).read()
        body = text[text.index("#define PFT_EXP_TAB_INIT"):]
        body = body[:body.index("\n\n")]
        got = [(int(a, 16), int(b, 16)) for a, b in re.findall(r"\{0x([0-9a-f]{16})ULL, 0x([0-9a-f]{16})ULL\}", body)]
        if got != tab:
            print("pft_cosh.h's table differs from the regenerated one")
            return 1
        print("pft_cosh.h's table equals the regenerated one (128 entries)")
        return 0
    print(literals(tab))
    return 0


if __name__ == "__main__":
    sys.exit(main())
