#!/usr/bin/env python3
"""Are the kernels of two device-only compiles of rtw_kernels.hip the same?

  hipcc <DEVICE + COMMON + INCLUDES of build.py> --offload-device-only -S \\
        -Rpass-analysis=kernel-resource-usage -x hip rtw_kernels.hip -o a.s 2> a.ru
  python profiles/select/compare_device_code.py a.s a.ru b.s b.ru

Compares the set of kernel symbols, each kernel's instruction stream (local
labels .LBB<n>_ lose their function number: instantiation order may differ)
and its kernel-resource-usage remarks (registers, spills, scratch, LDS,
occupancy).  Prints the kernel count and "identical", or the kernels that
differ; exits 1 when any does."""
import re
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    out = {}
    for n in names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(n), text, re.M | re.S)
        body = re.sub(r"[ \t]*;.*$", "", m.group(1), flags=re.M)  # comments (they cite BB<n>_ too)
        out[n] = re.sub(r"\.LBB\d+_", ".LBB_", body)
    return out


def usage(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def main(a_s, a_ru, b_s, b_ru):
    ka, kb = kernels(a_s), kernels(b_s)
    ua, ub = usage(a_ru), usage(b_ru)
    bad = [f"only in {a_s}: {n}" for n in sorted(set(ka) - set(kb))]
    bad += [f"only in {b_s}: {n}" for n in sorted(set(kb) - set(ka))]
    for n in sorted(set(ka) & set(kb)):
        if ka[n] != kb[n]:
            bad.append(f"instructions differ: {n}")
        if ua.get(n) != ub.get(n) or n not in ua:
            bad.append(f"resource usage differs: {n}: {ua.get(n)} vs {ub.get(n)}")
    print(f"{len(ka)} kernels vs {len(kb)} kernels:", "identical" if not bad else f"{len(bad)} differences")
    for b in bad:
        print("  " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
