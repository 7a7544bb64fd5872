"""Instruction count along ONE path through a stretch of a kernel's gfx950 ISA: region_census.py counts the text lines between two lines, which includes blocks the
path of interest never enters (the other side of a uniform branch, code of other phases the compiler placed in between).  This walks the listing from a line of the
kernel's body to the first line it reaches of a set of end lines (or the first branch back into the path walked so far: a loop), following every branch by a decision string:
usage: python tools/path_census.py usim.s '<mangled-name prefix>' FROM 'DECISIONS' [END ...]
DECISIONS: one letter per conditional branch met, in order -- t (taken) or n (not taken); beyond the string the walk stops and prints where, so that the string is
built one branch at a time with the listing at hand.  s_branch is followed.  Output: the branches met, then the instruction mix of the path (classes of region_census.py)."""
import collections, re, sys
path, key, lo, dec = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
ends = {int(x) for x in sys.argv[5:]}
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith(key) and ":" in l and l.split(":")[0].startswith(key))
end = next(i for i, l in enumerate(lines) if i > start and l.strip().startswith(".amdhsa_kernel"))
body = lines[start:end]
def is_inst(l):
    l = l.strip()
    return bool(l) and not l.startswith((".", ";", "//")) and not l.split(";")[0].strip().endswith(":")
labels = {l.split(":")[0].strip(): i for i, l in enumerate(body) if l.strip().startswith(".LBB") and ":" in l}
seq, i, d, seen = [], lo, 0, set()
while i < len(body):
    if i in ends and seq:
        print(f"reached end line {i}"); break
    l = body[i].strip()
    if not is_inst(l):
        i += 1; continue
    seq.append(l); seen.add(i)
    m = re.match(r"s_(c?)branch\w*\s+(\.LBB\S+)", l)
    if m:
        tgt = labels[m.group(2)]
        if not m.group(1):
            print(f"line {i}: {l} -> {tgt}")
            if tgt in seen or any(x in seen for x in range(tgt, min(tgt + 8, len(body)))): print("branch back into the path (a loop): stop"); break
            i = tgt; continue
        if d >= len(dec):
            print(f"line {i}: {l} (target line {tgt}) -- no decision left, stop"); break
        take = dec[d] == "t"; d += 1
        print(f"line {i}: {l} (target line {tgt}) {'taken' if take else 'not taken'}")
        if take:
            if any(x in seen for x in range(tgt, min(tgt + 8, len(body)))): print("branch back into the path (a loop): stop"); break
            i = tgt; continue
    i += 1
c = collections.Counter(x.split()[0] for x in seq)
grp = lambda f: sum(v for k, v in c.items() if f(k))
print(f"path from line {lo}: {len(seq)} instructions")
print(f"  plain moves {c['v_mov_b32_e32'] + c['v_mov_b64_e32']}; s_waitcnt {c['s_waitcnt']}; s_nop {c['s_nop']}; v_pk_* {grp(lambda k: k.startswith('v_pk_'))}; v_cndmask {grp(lambda k: k.startswith('v_cndmask'))}; "
      f"v_cmp* {grp(lambda k: k.startswith('v_cmp'))}; DPP {sum(1 for x in seq if 'dpp' in x.split()[0] or ' row_' in x or 'quad_perm' in x)}; "
      f"SALU without s_nop / s_waitcnt {grp(lambda k: k.startswith('s_') and k not in ('s_nop', 's_waitcnt'))}; LDS {grp(lambda k: k.startswith('ds_'))}; scratch {grp(lambda k: k.startswith('scratch_'))}")
print(f"  scalar fp32 VALU {grp(lambda k: re.match(r'v_(add|sub|mul|fma|fmac|fmamk|fmaak|max|min|rcp|rsq)_f32', k) is not None and 'dpp' not in k)}")
