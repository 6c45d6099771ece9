"""Device assembly of one source, kernel by kernel: which kernels of two .s files (as tools/device_asm_diff.sh writes
them with KEEP=dir) are byte-equal.  For a change that must leave some instantiations of a file alone while it edits
others -- the whole-file comparison of device_asm_diff.sh can only say that the file differs.

usage: tools/device_asm_kernels.py <this.s> <other.s> [regex]     (regex: only the kernels whose symbol matches)

Per kernel three pieces are compared: the body (from its label to its .Lfunc_end), its .amdhsa_kernel descriptor and
its entry of the amdhsa.kernels metadata (arguments, register and LDS use).  The compilation-unit id
(__hip_cuid_<hash>) and the function's index in its local labels (with the padding behind such a label) are masked.  Prints one line per kernel; exits 1 if a compared kernel differs or the two files do not
hold the same kernels.
"""
import re
import sys


def kernels(path):
    s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    # local labels carry the function's index in the file (.LBB<fn>_<block>, .Lfunc_end<fn>), which moves when an
    # instantiation is added before it; the block numbers stay
    s = re.sub(r"BB\d+_(\d+)", r"BB_\1", s)
    s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)
    # a label's trailing comment is padded to a column, so the padding moves with the index's number of digits
    s = re.sub(r"^(\.LBB_\d+:)[ \t]+;", r"\1 ;", s, flags=re.M)
    meta = re.split(r"^  - (?=\.agpr_count)", s.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0], flags=re.M)   # (not the file's trailer)
    out = {}
    for k in sorted(set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, re.M))):
        q = re.escape(k)
        body = re.search(r"^%s:.*?^\.Lfunc_end:" % q, s, re.M | re.S).group(0)
        desc = re.search(r"^\s*\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % q, s, re.M | re.S).group(0)
        mine = [m for m in meta if re.search(r"\.name:\s+%s\n" % q, m)]
        assert len(mine) == 1, (k, len(mine))
        out[k] = (body, desc, mine[0])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pick = re.compile(sys.argv[3] if len(sys.argv) > 3 else "")
    rc = 0
    if sorted(a) != sorted(b):
        print("the two files do not hold the same kernels")
        rc = 1
    for k in sorted(set(a) & set(b)):
        if not pick.search(k):
            continue
        same = a[k] == b[k]
        rc |= not same
        print(f"{'identical' if same else 'DIFFERS  '}  {k}  ({len(a[k][0].splitlines())} lines)")
    sys.exit(rc)


if __name__ == "__main__":
    main()
