"""usage: tools/kernel_stats_diff.py <kernel_stats.csv A> <kernel_stats.csv B> <steps> [name regex]: per-kernel launches and
microseconds PER STEP of two `rocprofv3 --kernel-trace --stats --output-format csv` runs of bench.py (steps = warm-up + timed
steps of the run; template arguments folded into one line per kernel), largest first, and the sum over all kernels."""
import collections
import csv
import re
import sys


def load(path):
    d = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        name = re.sub(r'\(.*', '', r['Name']).replace('void ', '').replace('mvd::', '')
        name = re.sub(r'<.*', '', name)
        c, t = d.get(name, (0, 0))
        d[name] = (c + int(r['Calls']), t + int(r['TotalDurationNs']))
    return d


def main():
    a, b, steps = load(sys.argv[1]), load(sys.argv[2]), float(sys.argv[3])
    pat = sys.argv[4] if len(sys.argv) > 4 else None
    names = sorted(set(a) | set(b), key=lambda n: -max(a.get(n, (0, 0))[1], b.get(n, (0, 0))[1]))
    print(f"{'kernel':28} {'A launches/step':>16} {'us/step':>9} {'B launches/step':>16} {'us/step':>9} {'B - A us':>9}")
    ta = tb = 0
    for n in names:
        ca, tta = a.get(n, (0, 0))
        cb, ttb = b.get(n, (0, 0))
        ta += tta
        tb += ttb
        if pat and not re.search(pat, n):
            continue
        print(f"{n:28} {ca / steps:16.2f} {tta / steps / 1e3:9.1f} {cb / steps:16.2f} {ttb / steps / 1e3:9.1f} "
              f"{(ttb - tta) / steps / 1e3:9.1f}")
    print(f"{'all kernels':28} {'':16} {ta / steps / 1e3:9.1f} {'':16} {tb / steps / 1e3:9.1f} {(tb - ta) / steps / 1e3:9.1f}")


if __name__ == "__main__":
    main()
