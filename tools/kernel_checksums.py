"""Per-kernel checksum of a device assembly listing: which kernels of a translation unit a change leaves instruction for instruction as they were.
usage: hipcc <the Makefile's flags> -S --cuda-device-only -o usim.s usim_api.hip ; python tools/kernel_checksums.py usim.s [other.s]
One listing: `sha256[:16]  instructions  demangled-ish name` per kernel (the body between the kernel's label and its .Lfunc_end, comments dropped).
Two listings: the kernels whose bodies differ, then the count of those that are the same."""
import hashlib, re, sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l.split(";")[0].rstrip() for l in lines[start + 1:end]]
        body = [l for l in body if l.strip()]
        insts = sum(1 for l in body if not l.strip().startswith(".") and not l.strip().endswith(":"))
        out[name] = (hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], insts)
    return out


a = kernels(sys.argv[1])
if len(sys.argv) < 3:
    for k, (h, n) in a.items():
        print(h, "%6d" % n, k)
    sys.exit(0)
b = kernels(sys.argv[2])
assert a.keys() == b.keys(), "the listings hold different kernels"
diff = [k for k in a if a[k] != b[k]]
for k in diff:
    print("differs  %s %6d -> %s %6d  %s" % (a[k][0], a[k][1], b[k][0], b[k][1], k))
print("%d kernels differ, %d are the same instruction for instruction" % (len(diff), len(a) - len(diff)))
