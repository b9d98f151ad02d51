"""Static instruction counts of one kernel in a gfx950 assembly listing (hipcc --save-temps, the *-gfx950.s file):
instructions before the first MFMA, between the first and the last MFMA, and after the last one in layout order, by class.
Static, per wave, in layout order: not executed counts (both sides of a branch are counted).
usage: python tools/isa_counts.py FILE.s k_fwd_wino3"""
import collections
import re
import sys


def klass(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "v_mov"
    if op.startswith("v_pk_"):
        return "v_pk"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return op
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"):
        return op
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "s_wait/nop"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, kern = sys.argv[1], sys.argv[2]
    body, inside = [], False
    for line in open(path):
        s = line.strip()
        if not inside:
            if re.match(r"^_Z\w*%s\w*:" % re.escape(kern), s):
                inside = True
            continue
        # a kernel may have several s_endpgm: the end-of-function marker ends it
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            break
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        body.append(s.split()[0])
    mf = [i for i, op in enumerate(body) if op.startswith("v_mfma")]
    parts = {"before the first MFMA": body[:mf[0]], "first to last MFMA": body[mf[0]:mf[-1] + 1],
             "after the last MFMA": body[mf[-1] + 1:]}
    print(f"{kern}: {len(body)} instructions, {len(mf)} MFMAs")
    for name, ops in parts.items():
        c = collections.Counter(klass(op) for op in ops)
        vec = c["v_mov"] + c["v_pk"] + c["valu"]
        print(f"  {name}: {len(ops)} instructions, {vec} vector (v_mov {c['v_mov']}, packed {c['v_pk']}, other {c['valu']}), "
              f"scalar {c['salu']}, barriers {c['s_barrier']}")
        for k in sorted(c):
            if k.startswith("ds_") or k.startswith("global_") or k.startswith("buffer_") or k.startswith("scratch_"):
                print(f"      {k:28s} {c[k]}")
        if name == "after the last MFMA":
            det = collections.Counter(op for op in ops if klass(op) == "valu")
            print("      vector detail: " + ", ".join(f"{k} {v}" for k, v in det.most_common(12)))


if __name__ == "__main__":
    main()
