#!/bin/bash
# Same-box A/B of render.draw between two TREES: `scripts/draw_ab.sh OLD_TREE [LOG]` runs scripts/draw_bench.py from OLD_TREE (a
# checkout of the commit to compare with, e.g. `git worktree add OLD_TREE HEAD~1`, its library built there with
# deepsvg_amd/csrc/build.sh) and from this tree in alternating rounds - old, new, three times - and prints, per size and
# variant of draw, the three medians of each side, their median, the range of the old side's runs and the difference of the
# medians; with LOG the summary is appended to it (profiles/draw_grad_bench.log holds one).
set -o pipefail
cd "$(dirname "$0")/.."
OLD=$(cd "$1" && pwd) || exit 2
LOG=$2
TMP=$(mktemp -d)
for round in 1 2 3; do
  (cd "$OLD" && timeout -k 10 180 python scripts/draw_bench.py --log "$TMP/old_$round.log" > /dev/null) || exit 1
  timeout -k 10 180 python scripts/draw_bench.py --log "$TMP/new_$round.log" > /dev/null || exit 1
done
python - "$TMP" "$LOG" <<'PY'
import glob, re, statistics, sys
tmp, log = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""


def medians(side):
    out = {}
    for path in sorted(glob.glob(f"{tmp}/{side}_*.log")):
        for m in re.finditer(r"size (\d+) (draw_fill|draw_mixed): ([\d.]+) us", open(path).read()):
            out.setdefault((int(m.group(1)), m.group(2)), []).append(float(m.group(3)))
    return out


old, new = medians("old"), medians("new")
lines = ["", "render.draw of another tree (old) against this tree (new) on the same box: scripts/draw_ab.sh, scripts/draw_bench.py from "
         "either tree in alternating rounds (old, new, three times), each run the median of 7 rounds of 50 calls; microseconds: the "
         "three runs, their median, [the range of the old side's runs]"]
for key in sorted(old):
    o, n = old[key], new[key]
    lines.append(f"size {key[0]} {key[1]}: old {' '.join(f'{v:.1f}' for v in o)} median {statistics.median(o):.1f} [spread "
                 f"{max(o) - min(o):.1f}]; new {' '.join(f'{v:.1f}' for v in n)} median {statistics.median(n):.1f}; difference of the "
                 f"medians {statistics.median(n) - statistics.median(o):+.1f} us")
text = "\n".join(lines)
print(text)
if log:
    with open(log, "a") as f:
        f.write(text + "\n")
PY
rm -rf "$TMP"
