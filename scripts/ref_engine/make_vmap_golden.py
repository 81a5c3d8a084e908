"""Golden vectors of seam-map loading (include/lqr_vmap.h), produced by EXECUTING the reference author's own liblqr build on inputs
generated here, as make_energy_golden.py does for the energy read-outs.  BUILD CONTAINER ONLY; only the DATA this writes
(tests/golden/vmap/*.npz + MANIFEST.json) travels.

    python scripts/ref_engine/make_vmap_golden.py [NAME ...]     (names: only these vectors are recorded again)

tests/vmap_cases.py holds the specs, the driver and the numpy model.  Every vector records the input image, the map (a "carve" map is
dumped by a genuine carver of the same image here), every call's return value and the getters after it, the image after every resize,
the map dumped again after every load, and the carver's list after lqr_vmap_internal_dump.  Both modes are run ("sse": the mode
bit-exact refers to; and the exe as shipped); the heap is checked after each; and the model is compared HERE with every
image recorded while the carver shows the loaded map alone (model_equal in the manifest).
"""
import hashlib, json, os, sys, time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
import numpy as np
import imgtype_cases as IT, vmap_cases as VC
import ref_engine as R

OUT = os.environ.get("VMAP_OUT") or os.path.join(ROOT, "tests", "golden", "vmap")


def bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8) if a.dtype.kind == "f" else a


def vmap_api(mode, spec):
    if mode != "sse":
        return R.RefApi(0x37f)
    only = tuple(f for f in R.FLOAT_ONLY if not (spec["depth"] == 3 and f == "lqr_carver_inflate"))      # (as make_ref_golden.coldepth_api)
    return R.RefApi(0x27f, float24_only=only)


def one(task):
    name, spec = task
    img, extra = VC.make_input(spec)
    res = {}
    for mode in ("sse", "shipped"):
        a = vmap_api(mode, spec)
        try:
            t0 = time.time()
            out = VC.run(a, R.RefCarver, spec, img, extra)
            res[mode] = (out, a.r.heap_check(), time.time() - t0)
        finally:
            a.close()
    out, heap, secs = res["sse"]
    other, heap_shipped = res["shipped"][0], res["shipped"][1]
    same = out.keys() == other.keys() and all(np.array_equal(bits(out[k]), bits(other[k])) for k in out)
    compared, differ = VC.model_check(spec, img, out)
    compared_shipped, differ_shipped = VC.model_check(spec, img, other)
    fn = "vmap_%s.npz" % name
    np.savez_compressed(os.path.join(OUT, fn), **dict(out, img=img, spec=np.array(json.dumps(spec, sort_keys=True))))
    rec = json.loads(str(out["record"]))
    m = dict(data=out["map"], depth=rec["map_meta"][0], orientation=rec["map_meta"][1])
    return dict(name=name, spec=spec, heap=[heap["bad"], heap["freed_bad"]], heap_shipped=[heap_shipped["bad"], heap_shipped["freed_bad"]],
                same_as_shipped=bool(same), model_compared=compared, model_equal=not differ, model_differs=differ,
                model_equal_shipped=not differ_shipped, rets=rec["rets"], map_meta=rec["map_meta"], map_valid=bool(VC.valid_map(m, spec["w"], spec["h"])),
                final=rec["getters"][-1], seconds=round(secs, 2), file=fn)


def main(only=(), jobs=8):
    os.makedirs(OUT, exist_ok=True)
    R.build_runner()
    cases = VC.cases() + VC.finding_cases()
    n_findings = len(VC.finding_cases())
    todo = [t for t in cases if not only or t[0] in only]
    assert len(todo) == (len(only) or len(cases)), "unknown vector name"
    man_path = os.path.join(OUT, "MANIFEST.json")
    kept = {}
    if only:
        old = json.load(open(man_path))
        kept = {e["name"]: e for e in old["vectors"] + old["findings"] if e["name"] not in only}
    else:
        for f in os.listdir(OUT):
            if f.endswith(".npz"):
                os.remove(os.path.join(OUT, f))
    with ProcessPoolExecutor(jobs) as ex:
        made = list(ex.map(one, todo))
    for e in made:
        with open(os.path.join(OUT, e["file"]), "rb") as f:
            e["sha256"] = hashlib.sha256(f.read()).hexdigest()
        kept[e["name"]] = e
    entries = [kept[name] for name, _ in cases]
    man = dict(source="gimp-lqr-plugin.exe (liblqr 0.4.1 statically linked), executed by scripts/ref_engine/refrun.c",
               exe_sha256=hashlib.sha256(R.exe_bytes()).hexdigest(),
               mode="sse: x87 control word 0x27f, float-only DP functions under 0x07f",
               rules=VC.RULES_NOTE, vectors=entries[:len(entries) - n_findings], findings=entries[len(entries) - n_findings:])
    with open(man_path, "w") as f:
        json.dump(man, f, indent=1)
    sizes = [os.path.getsize(os.path.join(OUT, e["file"])) for e in entries]
    assert max(sizes) <= IT.MAX_FILE, "a vector is over the file limit"
    print("vmap: %d vectors (%d recorded now), heap clean %d (as shipped %d), model equal to genuine on %d (%d images compared; as shipped: "
          "equal on %d), same as shipped %d; largest file %d B, total %d B" % (
              len(entries), len(made), sum(e["heap"] == [0, 0] for e in entries), sum(e["heap_shipped"] == [0, 0] for e in entries),
              sum(e["model_equal"] for e in entries), sum(e["model_compared"] for e in entries), sum(e["model_equal_shipped"] for e in entries),
              sum(e["same_as_shipped"] for e in entries), max(sizes), sum(sizes)))
    for e in entries:
        if not e["model_equal"] or e["heap"] != [0, 0] or e["heap_shipped"] != [0, 0]:
            print("  FINDING %s: model differs on %s, heap %s (as shipped %s)" % (e["name"], e["model_differs"], e["heap"], e["heap_shipped"]))
        print("   %-24s rets %s final %s" % (e["name"], e["rets"], e["final"]))


if __name__ == "__main__":
    main(only=sys.argv[1:])
