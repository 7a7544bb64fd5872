"""Static census of one stretch of a kernel's gfx950 ISA, by text lines of the kernel's body: the instruction mix between two lines (for instance from the s_barrier of a
hand-off to the head of a loop).  Without the two lines it lists the kernel's s_barrier lines and its loops (backward branches) with their instruction counts, from which
the stretch is chosen.
usage: hipcc ... -S --cuda-device-only -o usim.s usim_api.hip ; python tools/region_census.py usim.s '<mangled-name prefix>' [FROM TO [dump]]
The contact set-up of the split kernel's lattice role (profiles/contact_setup/): prefix _ZN4usim18usim_step32_kernelILb1ELi16ELb0EE, FROM = the third s_barrier (hand-off
(2)), TO = the head of the first Jacobi loop (the loop of about 190 instructions; the loops stand in the order >= 5 contacts, 4, 3, 2, 1)."""
import collections, re, sys
path, key = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith(key) and ":" in l and l.split(":")[0].startswith(key))
end = next(i for i, l in enumerate(lines) if i > start and l.strip().startswith(".amdhsa_kernel"))
body = lines[start:end]
def is_inst(l):
    l = l.strip()
    return bool(l) and not l.startswith((".", ";", "//")) and not l.split(";")[0].strip().endswith(":")
bars = [i for i, l in enumerate(body) if is_inst(l) and l.split()[0] == "s_barrier"]
labels = {l.split(":")[0].strip(): i for i, l in enumerate(body) if l.strip().startswith(".LBB") and ":" in l}
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\w*\s+(\.LBB\S+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], sum(1 for x in body[labels[m.group(1)]:i + 1] if is_inst(x))))
print("s_barrier at lines", bars)
print("loops of 100 .. 300 instructions (head line, instructions)", [x for x in sorted(loops) if 100 <= x[1] <= 300])
if len(sys.argv) < 5:
    sys.exit(0)
lo, hi = int(sys.argv[3]), int(sys.argv[4])
seg = [l.strip() for l in body[lo:hi] if is_inst(l)]
c = collections.Counter(x.split()[0] for x in seg)
grp = lambda f: sum(v for k, v in c.items() if f(k))
b64 = c["v_mov_b64"] + c["v_mov_b64_e32"]
print(f"lines {lo} .. {hi}: {len(seg)} instructions")
print(f"  plain moves {c['v_mov_b32_e32'] + b64} (v_mov_b32_e32 {c['v_mov_b32_e32']}, v_mov_b64 {b64}); s_waitcnt {c['s_waitcnt']}; s_nop {c['s_nop']}")
print(f"  LDS reads: ds_read_b32 {c['ds_read_b32']}, ds_read2_b32 {c['ds_read2_b32']}, ds_read_b64 {c['ds_read_b64']}, ds_read2_b64 {c['ds_read2_b64']}, ds_read_b128 {c['ds_read_b128']}; LDS writes {grp(lambda k: k.startswith('ds_write'))}")
print(f"  v_pk_* {grp(lambda k: k.startswith('v_pk_'))}; v_cndmask {grp(lambda k: k.startswith('v_cndmask'))}; DPP {sum(1 for x in seg if 'dpp' in x.split()[0] or ' row_' in x or 'quad_perm' in x)}; "
      f"v_cmp* {grp(lambda k: k.startswith('v_cmp'))}; v_readlane {c['v_readlane_b32']}; SALU without s_nop / s_waitcnt {grp(lambda k: k.startswith('s_') and k not in ('s_nop', 's_waitcnt'))}; "
      f"scratch {grp(lambda k: k.startswith('scratch_'))}")
for k, v in c.most_common(24):
    print(f"    {k:28s} {v}")
if len(sys.argv) > 5 and sys.argv[5] == "dump":
    print("\n".join(body[lo:hi]))
