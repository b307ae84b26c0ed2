"""large_tree_select.jsonl (run_large_tree_select.sh) -> the table of large_tree_select.md: per (package, B, case) the
median over the processes' medians and the min .. max over all repeats, kernel times by HIP events in ms."""
import json
import sys
from collections import defaultdict

rows = defaultdict(lambda: defaultdict(list))
meta = {}
for line in open(sys.argv[1]):
    line = line.strip()
    if not line.startswith("{"):
        continue
    d = json.loads(line)
    key = (d["case"], d["B"], d["tag"])
    meta[key] = {k: d[k] for k in ("Q", "pairs") if k in d}
    for k, v in d.items():
        if k.endswith("_ms"):
            rows[key][k].append(v if isinstance(v, dict) else {"median": v, "min": v, "max": v})
print("| case | B | package | Q | pairs | kernel family | median ms | min .. max ms |")
print("|---|---|---|---|---|---|---|---|")
for key in sorted(rows):
    for fam, vs in sorted(rows[key].items()):
        meds = sorted(v["median"] for v in vs)
        print("| %s | %d | %s | %s | %s | %s | %.3f | %.3f .. %.3f |" % (
            key[0], key[1], key[2], meta[key].get("Q", ""), meta[key].get("pairs", ""), fam[:-3],
            meds[len(meds) // 2], min(v["min"] for v in vs), max(v["max"] for v in vs)))
