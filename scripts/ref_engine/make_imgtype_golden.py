"""Golden vectors of the image-type surface (include/lqr_imagetype.h), produced by EXECUTING the reference author's own liblqr
build on inputs generated here, as make_ref_golden.py does for the colour depths.  BUILD CONTAINER ONLY; only the DATA this writes
(tests/golden/imgtype/*.npz + MANIFEST.json) travels.

    python scripts/ref_engine/make_imgtype_golden.py [NAME ...]     (names: only these vectors are recorded again)

tests/imgtype_cases.py holds the specs (cases(), mid_cases()) and the driver.  Every vector records what a colour-depth vector
records plus the setters' return values; for PLANE_CASES also the genuine lqr_carver_read_brightness / lqr_carver_read_luma of
every input pixel (in_read_bright, in_read_luma: float64), which the CPU suite compares with imgtype_cases.model_value.
"""
import hashlib, json, os, sys, time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
import numpy as np
import coldepth_cases as CD, imgtype_cases as IT
import ref_engine as R
from make_ref_golden import coldepth_api

OUT = os.environ.get("IMGTYPE_OUT") or os.path.join(ROOT, "tests", "golden", "imgtype")


def bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8) if a.dtype.kind == "f" else a


def one(task):
    name, spec = task
    img, extra = CD.make_input(spec)
    res = {}
    for mode in ("sse", "shipped"):
        a = coldepth_api(mode, spec)
        try:
            t0 = time.time()
            out = IT.run(a, R.RefCarver, spec, img, extra)
            res[mode] = (out, a.r.heap_check(), time.time() - t0)
        finally:
            a.close()
    out, heap, secs = res["sse"]
    other = res["shipped"][0]
    same = out.keys() == other.keys() and all(np.array_equal(bits(out[k]), bits(other[k])) for k in out)
    arrays = dict(out, img=img, spec=np.array(json.dumps(spec, sort_keys=True)))
    for k, v in extra.items():
        arrays["in_" + k] = v
    planes = name in IT.PLANE_CASES
    if planes:
        a = coldepth_api("sse", spec)
        try:
            c = R.RefCarver.from_ext(a, img, spec["depth"])
            for op in IT.initial_ops(spec):
                IT._apply(c, op)
            arrays["in_read_bright"], arrays["in_read_luma"] = c.read_planes()
            c.destroy()
        finally:
            a.close()
    fn = "imgtype_%s.npz" % name
    np.savez_compressed(os.path.join(OUT, fn), **arrays)
    rec = json.loads(str(out["record"]))
    return dict(name=name, spec=spec, heap=[heap["bad"], heap["freed_bad"]], same_as_shipped=bool(same), input_unchanged=rec.get("input_unchanged"),
                rets=rec["rets"], type_rets=rec["type_rets"], default_type=rec["default_type"], read_planes=planes, seconds=round(secs, 2), file=fn)


def main(only=(), jobs=8):
    """every vector, or only the named ones (the others' files and manifest entries stay as they are)"""
    os.makedirs(OUT, exist_ok=True)
    R.build_runner()
    small, mid = IT.cases(), IT.mid_cases()
    todo = [t for t in small + mid if not only or t[0] in only]
    assert len(todo) == (len(only) or len(small + mid)), "unknown vector name"
    man_path = os.path.join(OUT, "MANIFEST.json")
    kept = {}
    if only:
        old = json.load(open(man_path))
        kept = {e["name"]: e for e in old["vectors"] + old["mid"] if e["name"] not in only}
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
    entries = [kept[name] for name, _ in small + mid]
    man = dict(source="gimp-lqr-plugin.exe (liblqr 0.4.1 statically linked), executed by scripts/ref_engine/refrun.c",
               exe_sha256=hashlib.sha256(R.exe_bytes()).hexdigest(),
               mode="sse: x87 control word 0x27f, float-only DP functions under 0x07f (64F cases: lqr_carver_inflate under 0x27f)",
               vectors=entries[:len(small)], mid=entries[len(small):])
    with open(man_path, "w") as f:
        json.dump(man, f, indent=1)
    sizes = [os.path.getsize(os.path.join(OUT, e["file"])) for e in entries]
    assert max(sizes) <= IT.MAX_FILE, "a vector is over the file limit"
    print("imgtype: %d + %d vectors (%d recorded now), heap clean %d, all resizes LQR_OK %d, same as shipped %d, %d read-plane sets; largest file %d B, total %d B" % (
        len(small), len(mid), len(made), sum(e["heap"] == [0, 0] for e in entries), sum(all(r == 1 for r in e["rets"]) for e in entries),
        sum(e["same_as_shipped"] for e in entries), sum(e["read_planes"] for e in entries), max(sizes), sum(sizes)))


if __name__ == "__main__":
    main(only=sys.argv[1:])
