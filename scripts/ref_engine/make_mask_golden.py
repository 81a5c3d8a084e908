"""Golden vectors of the computed-mask surface (include/lqr_masks.h), produced by EXECUTING the reference author's own liblqr build
on inputs generated here, as make_imgtype_golden.py does for the image types.  BUILD CONTAINER ONLY; only the DATA this writes
(tests/golden/masks/*.npz + MANIFEST.json) travels.

    python scripts/ref_engine/make_mask_golden.py [NAME ...]     (names: only these vectors are recorded again)

tests/mask_cases.py holds the specs, the driver and the numpy model.  Every vector records the input image, every call's return
value, the genuine bias and rigidity planes after the mask calls (read out of the genuine struct), the energy plane, and the carved
image and visibility map after each resize that follows.  Both modes are run ("sse": the mode bit-exact refers to; and
the exe as shipped); the heap is checked after each; and every recorded plane is compared with mask_cases.Model HERE, so that a
vector on which the genuine build and the model differ is found when it is made (model_equal in the manifest).
"""
import hashlib, json, os, sys, time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
import numpy as np
import imgtype_cases as IT, mask_cases as MC
import ref_engine as R
from make_ref_golden import coldepth_api

OUT = os.environ.get("MASKS_OUT") or os.path.join(ROOT, "tests", "golden", "masks")


def bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8) if a.dtype.kind == "f" else a


def model_check(spec, out):
    """(planes compared, planes that differ): mask_cases.Model against the recorded planes, snapshots and final ones"""
    _, extra = MC.make_input(spec)
    m = MC.Model(spec, extra["masks"])
    rec = json.loads(str(out["record"]))
    compared, differ = 0, []

    def check(key_b, key_r):
        nonlocal compared
        if not m.valid:
            m.adopt(out[key_b], out[key_r])
            return
        for which, key in (("bias", key_b), ("rig", key_r)):
            compared += 1
            if not np.array_equal(bits(m.plane(which)), bits(out[key])):
                differ.append(key)

    for i, op in enumerate(spec["ops"]):
        if op[0] == "aux":
            want = 0
        else:
            want = m.apply(op)
        kind = op[1] if op[0] == "aux" else op[0]
        if kind == "planes":
            check("bias@%d" % i, "rig@%d" % i)
        elif kind in ("bias_xy", "rig_xy"):
            assert [v for v, _ in rec["rets"][i]] == [want], (spec["ops"][i], rec["rets"][i])
        else:
            assert rec["rets"][i] == want, (spec["ops"][i], rec["rets"][i], want)
    if "bias" in out and m.valid:
        check("bias", "rig")
    return compared, differ


def one(task):
    name, spec = task
    img, extra = MC.make_input(spec)
    res = {}
    for mode in ("sse", "shipped"):
        a = coldepth_api(mode, spec)
        try:
            t0 = time.time()
            out = MC.run(a, R.RefCarver, spec, img, extra)
            res[mode] = (out, a.r.heap_check(), time.time() - t0)
        finally:
            a.close()
    out, heap, secs = res["sse"]
    other = res["shipped"][0]
    same = out.keys() == other.keys() and all(np.array_equal(bits(out[k]), bits(other[k])) for k in out)
    heap_shipped = res["shipped"][1]
    compared, differ = model_check(spec, out)
    finding = name in dict(MC.finding_cases())
    swapped = model_check(MC.swapped_offsets(spec), out)[1] if finding else None
    fn = "masks_%s.npz" % name
    np.savez_compressed(os.path.join(OUT, fn), **dict(out, img=img, spec=np.array(json.dumps(spec, sort_keys=True))))
    rec = json.loads(str(out["record"]))
    return dict(name=name, spec=spec, heap=[heap["bad"], heap["freed_bad"]], heap_shipped=[heap_shipped["bad"], heap_shipped["freed_bad"]],
                same_as_shipped=bool(same), model_planes=compared, model_equal=not differ, model_differs=differ, rets=rec["rets"],
                step_rets=rec["step_rets"], planes=("bias" in out), seconds=round(secs, 2), file=fn,
                **(dict(swapped_offsets_model_equal=not swapped) if finding else {}))


def main(only=(), jobs=8):
    os.makedirs(OUT, exist_ok=True)
    R.build_runner()
    cases = MC.cases() + MC.finding_cases()
    n_findings = len(MC.finding_cases())
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
               mode="sse: x87 control word 0x27f, float-only DP functions under 0x07f; the mask calls themselves run under 0x27f",
               rounding=MC.ROUNDING_NOTE, vectors=entries[:len(entries) - n_findings], findings=entries[len(entries) - n_findings:])
    with open(man_path, "w") as f:
        json.dump(man, f, indent=1)
    sizes = [os.path.getsize(os.path.join(OUT, e["file"])) for e in entries]
    assert max(sizes) <= IT.MAX_FILE, "a vector is over the file limit"
    print("masks: %d vectors (%d recorded now), heap clean %d (as shipped %d), model equal to genuine on %d (%d planes compared), all resizes LQR_OK %d, "
          "same as shipped %d; largest file %d B, total %d B" % (
              len(entries), len(made), sum(e["heap"] == [0, 0] for e in entries), sum(e["heap_shipped"] == [0, 0] for e in entries),
              sum(e["model_equal"] for e in entries), sum(e["model_planes"] for e in entries),
              sum(all(r == 1 for r in e["step_rets"]) for e in entries), sum(e["same_as_shipped"] for e in entries), max(sizes), sum(sizes)))
    for e in entries:
        if not e["model_equal"] or e["heap"] != [0, 0]:
            print("  FINDING %s: model differs on %s, heap %s%s" % (e["name"], e["model_differs"], e["heap"],
                  "; equal to the model with x_off and y_off exchanged: %s" % e["swapped_offsets_model_equal"] if "swapped_offsets_model_equal" in e else ""))


if __name__ == "__main__":
    main(only=sys.argv[1:])
