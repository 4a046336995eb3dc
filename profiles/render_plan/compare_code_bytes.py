#!/usr/bin/env python3
"""Are the kernels of two gfx950 code objects the same bytes?

  hipcc <DEVICE + COMMON + INCLUDES of build.py> --offload-device-only -c -x hip rtw_kernels.hip -o a.co
  clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=a.co --output=a.elf
  python profiles/render_plan/compare_code_bytes.py a.elf b.elf

Reads the two linked code objects' symbol tables and compares, symbol by
symbol, the bytes of every function (STT_FUNC: the kernels and what they
call) and of every kernel descriptor (<kernel>.kd: registers, LDS, scratch,
kernarg bytes), wherever the linker put them.  Two things depend on where a
kernel sits in .text and are set aside: the descriptor's
kernel_code_entry_byte_offset (bytes 16..23), and 32-bit pc-relative literals
in the code (the distance to a table in .rodata or to a called function).
The latter show as differing dwords that, per pair of moved symbols, all
change by the same amount: the tool counts them and lists the distinct
amounts.  Exits 1 when the symbol sets, a function's size, or a descriptor
(offset aside) differ."""
import struct
import sys


def symbols(path):
    b = open(path, "rb").read()
    assert b[:4] == b"\x7fELF" and b[4] == 2, path
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", b, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + k * shentsize) for k in range(shnum)]
    out = {}
    for s in sec:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        strtab = sec[s[6]]
        for k in range(s[5] // s[9]):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", b, s[4] + k * s[9])
            kind = info & 15
            if kind not in (1, 2) or size == 0 or shndx == 0 or shndx >= len(sec):
                continue
            n = b[strtab[4] + name:b.index(b"\0", strtab[4] + name)].decode()
            if kind == 1 and not n.endswith(".kd"):  # objects: the kernel descriptors only
                continue
            at = sec[shndx][4] + value - sec[shndx][3]
            out[n] = b[at:at + size]
    return out


def main(a, b):
    sa, sb = symbols(a), symbols(b)
    bad = [f"only in {a}: {n}" for n in sorted(set(sa) - set(sb))] + [f"only in {b}: {n}" for n in sorted(set(sb) - set(sa))]
    moved_fns, moved_dwords, deltas = 0, 0, {}
    for n in sorted(set(sa) & set(sb)):
        x, y = sa[n], sb[n]
        if len(x) != len(y):
            bad.append(f"size differs: {n}: {len(x)} vs {len(y)}")
        elif n.endswith(".kd"):
            if x[:16] + x[24:] != y[:16] + y[24:]:
                bad.append(f"descriptor differs: {n}")
        elif x != y:
            d = [i for i in range(0, len(x), 4) if x[i:i + 4] != y[i:i + 4]]
            moved_fns, moved_dwords = moved_fns + 1, moved_dwords + len(d)
            for i in d:
                k = struct.unpack_from("<i", y, i)[0] - struct.unpack_from("<i", x, i)[0]
                deltas[k] = deltas.get(k, 0) + 1
    nk = sum(n.endswith(".kd") for n in sa)
    print(f"{len(sa) - nk} functions and {nk} kernel descriptors, {sum(len(v) for n, v in sa.items() if not n.endswith('.kd'))} "
          f"bytes of code:", "same symbols, sizes and descriptors" if not bad else f"{len(bad)} differences")
    print(f"  {len(sa) - nk - moved_fns} functions byte-identical; {moved_fns} differ in {moved_dwords} dwords in all, "
          f"each by one of {len(deltas)} amounts: " + ", ".join(f"{k:+d} x{v}" for k, v in sorted(deltas.items(), key=lambda kv: -kv[1])))
    for x in bad:
        print("  " + x)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
