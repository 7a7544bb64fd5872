"""Static census of one kernel's gfx950 ISA: instruction mix, spill traffic (v_readlane / v_writelane of spilled SGPRs, scratch), and the same per loop
(backward branches), so that what sits inside the 256-step loop can be told from what runs once per launch.
usage: hipcc ... -S --cuda-device-only -o usim.s usim_api.hip ; python tools/isa_census.py usim.s '<mangled-name prefix>' [LO HI]
With LO HI every loop of LO..HI instructions is listed too, in program order, with its mix of packed, DPP and move instructions (the Jacobi passes of the contact solve:
150 250; in the split kernel they stand in the order >= 5 contacts, 4, 3, 2, 1)."""
import collections, re, sys
path, key = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith(key) and ": " in l and l.split(":")[0].startswith(key))
end = next(i for i, l in enumerate(lines) if i > start and l.strip().startswith(".amdhsa_kernel"))
body = lines[start:end]
def is_inst(l):
    l = l.strip()
    return bool(l) and not l.startswith((".", ";", "//")) and not l.split(";")[0].strip().endswith(":")
def census(seg):
    c = collections.Counter(l.split()[0] for l in seg if is_inst(l))
    return c
WATCH = ("v_readlane_b32", "v_writelane_b32", "s_nop", "scratch_load_dword", "scratch_store_dword", "s_barrier")
c = census(body)
print(f"kernel: {sum(c.values())} instructions;", ", ".join(f"{k} {c[k]}" for k in WATCH), "; vector", sum(v for k, v in c.items() if k.startswith("v_")), "; dpp", sum(1 for l in body if is_inst(l) and "dpp" in l.split()[0] or " row_" in l or "quad_perm" in l))
labels = {l.split(":")[0].strip(): i for i, l in enumerate(body) if l.strip().startswith(".LBB") and ":" in l}
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\w*\s+(\.LBB\S+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], i))
loops.sort(key=lambda x: x[0] - x[1])
for a, b in loops[:8]:
    cc = census(body[a:b + 1])
    print(f"  loop lines {a}-{b}: {sum(cc.values())} instructions;", ", ".join(f"{k} {cc[k]}" for k in WATCH))
if len(sys.argv) > 4:
    lo, hi = int(sys.argv[3]), int(sys.argv[4])
    for a, b in sorted(loops):
        seg = [l.strip() for l in body[a:b + 1] if is_inst(l)]
        if lo <= len(seg) <= hi:
            n = lambda f: sum(1 for x in seg if f(x))
            dpp = lambda x: "dpp" in x.split()[0] or " row_" in x or "quad_perm" in x
            print(f"  loop lines {a}-{b}: {len(seg)} instructions; v_pk_* {n(lambda x: x.startswith('v_pk_'))}, dpp {n(dpp)} (v_mov_b32_dpp {n(lambda x: x.startswith('v_mov') and dpp(x))}),"
                  f" v_mov* {n(lambda x: x.startswith('v_mov'))}, v_cndmask {n(lambda x: x.startswith('v_cndmask'))}, s_nop {n(lambda x: x.startswith('s_nop'))},"
                  f" other SALU {n(lambda x: x.startswith('s_') and not x.startswith('s_nop'))}")
