"""Golden vectors of the carver-control calls (include/lqr_control.h: lqr_carver_cancel and the five small calls), produced by EXECUTING
the reference author's own liblqr build on inputs generated here, as make_vmap_golden.py does for seam-map loading.  BUILD CONTAINER
ONLY; only the DATA this writes (tests/golden/control/*.npz + MANIFEST.json) travels.

    python scripts/ref_engine/make_control_golden.py

tests/control_cases.py holds the specs, the driver and the engine's rules as a model.  lqr_carver_cancel is called from inside a resize
by the runner's update callback (refrun.c, OP_HOOK), which is where a caller's progress callback -- or its other thread -- calls it.
Every vector records every call's return value, the getters and the number of progress events after it, the event list, the images after
every resize, the maps dumped, and the heap check.  The manifest holds, per vector, where the recorded values differ from what the
engine's rules predict (tests/test_control_golden.py: empty for the vectors, named findings for the rest).
"""
import hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
import numpy as np
import control_cases as CC
import ref_engine as R

OUT = os.environ.get("CONTROL_OUT") or os.path.join(ROOT, "tests", "golden", "control")
MAX_FILE = 256 << 10


def differences(spec, rec):
    """where the genuine record leaves the engine's rules: a list of short strings"""
    p = CC.predict(spec)
    out = []
    for i, op in enumerate(spec["ops"]):
        if p["rets"][i] is not None and rec["rets"][i] != p["rets"][i]:
            out.append("ret@%d %s: genuine %s, rules %s" % (i, op[0], rec["rets"][i], p["rets"][i]))
        if rec["n_events"][i] != p["n_events"][i]:
            out.append("events@%d %s: genuine %d, rules %d" % (i, op[0], rec["n_events"][i], p["n_events"][i]))
        g = rec["getters"][i]
        if (g["width"], g["height"]) != tuple(p["sizes"][i]):
            out.append("size@%d %s: genuine %dx%d, rules %dx%d" % ((i, op[0], g["width"], g["height"]) + tuple(p["sizes"][i])))
    if rec["hooks"] != p["hooks"]:
        out.append("armed calls: genuine %s, rules %s" % (rec["hooks"], p["hooks"]))
    return out


def one(name, spec):
    img, aux = CC.make_input(spec)
    res = {}
    for mode in ("sse", "shipped"):
        a = R.RefApi(0x27f, float24=True) if mode == "sse" else R.RefApi(0x37f)
        try:
            out = CC.run(a, R.RefCarver, spec, img, aux)
            res[mode] = (out, a.r.heap_check())
        finally:
            a.close()
    out, heap = res["sse"]
    rec, rec_shipped = json.loads(str(out["record"])), json.loads(str(res["shipped"][0]["record"]))
    fn = "control_%s.npz" % name
    np.savez_compressed(os.path.join(OUT, fn), **dict(out, img=img, spec=np.array(json.dumps(spec, sort_keys=True))))
    return dict(name=name, spec=spec, heap=[heap["bad"], heap["freed_bad"]], heap_shipped=[res["shipped"][1]["bad"], res["shipped"][1]["freed_bad"]],
                rets=rec["rets"], rets_shipped_same=rec["rets"] == rec_shipped["rets"] and rec["n_events"] == rec_shipped["n_events"],
                hooks=rec["hooks"], n_events=rec["n_events"], final=rec["getters"][-1], differs_from_rules=differences(spec, rec), file=fn)


def main():
    os.makedirs(OUT, exist_ok=True)
    R.build_runner()
    for f in os.listdir(OUT):
        if f.endswith(".npz"):
            os.remove(os.path.join(OUT, f))
    vectors = [one(n, s) for n, s in CC.cases()]
    findings = [one(n, s) for n, s in CC.finding_cases()]
    for e in vectors + findings:
        with open(os.path.join(OUT, e["file"]), "rb") as f:
            data = f.read()
        e["sha256"] = hashlib.sha256(data).hexdigest()
        assert len(data) <= MAX_FILE, e["file"]
    for e in findings:
        e["finding"] = "half_built_state"
    man = dict(source="gimp-lqr-plugin.exe (liblqr 0.4.1 statically linked), executed by scripts/ref_engine/refrun.c",
               exe_sha256=hashlib.sha256(R.exe_bytes()).hexdigest(),
               mode="sse: x87 control word 0x27f, float-only DP functions under 0x07f",
               rules=CC.RULES_NOTE, gradient_to_builtin={str(k): v for k, v in CC.GRADIENT_TO_BUILTIN.items()},
               vectors=vectors, findings=findings)
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump(man, f, indent=1)
    for e in vectors + findings:
        print("%-28s rets %s hooks %s heap %s" % (e["name"], e["rets"], e["hooks"], e["heap"]))
        for d in e["differs_from_rules"]:
            print("      differs: " + d)
    print("control: %d vectors, %d findings, %d B" % (len(vectors), len(findings), sum(os.path.getsize(os.path.join(OUT, e["file"])) for e in vectors + findings)))


if __name__ == "__main__":
    main()
