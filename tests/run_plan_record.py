"""tests/golden/run_plan_table.json, the recorded decisions of hb_runplan.hpp, for the tests that read it (test_host_logic.py, test_gpu_runplan.py)."""
import os


def recorded_run_plan():
    """tests/golden/run_plan_table.json as {stage: {key: outcome}}, the keys in the order of the stage's dims (the first varies slowest)."""
    import itertools
    import json
    table = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_plan_table.json")))
    out = {}
    for stage, rec in table.items():
        if stage != "about":
            keys = [" ".join(str(x) for x in t) for t in itertools.product(*[v for _, v in rec["dims"]])]
            vals = [rec["outcomes"][i] for i, cnt in zip(rec["runs"][0::2], rec["runs"][1::2]) for _ in range(cnt)]
            assert len(keys) == len(vals), stage
            out[stage] = dict(zip(keys, vals))
    return out


def recorded_matvec_plan():
    """tests/golden/matvec_plan_table.json, the recorded decisions of hb_matvecplan.hpp (for test_host_logic.py and test_gpu_matvecplan.py), as
    {stage: {key: outcome}}. A stage's outcome is its fields joined by blanks; a field is recorded over the dims it depends on only."""
    import itertools
    import json
    table = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matvec_plan_table.json")))
    out = {}
    for stage, rec in table.items():
        if stage == "about":
            continue
        names, columns = [d for d, _ in rec["dims"]], []
        for f in rec["fields"]:
            at = [names.index(d) for d in f["over"]]
            vals = [f["outcomes"][i] for i, cnt in zip(f["runs"][0::2], f["runs"][1::2]) for _ in range(cnt)]
            keys = list(itertools.product(*[rec["dims"][i][1] for i in at]))
            assert len(keys) == len(vals), (stage, f["name"])
            columns.append((at, dict(zip(keys, vals))))
        out[stage] = {" ".join(str(x) for x in t): " ".join(col[tuple(t[i] for i in at)] for at, col in columns)
                      for t in itertools.product(*[v for _, v in rec["dims"]])}
    return out
