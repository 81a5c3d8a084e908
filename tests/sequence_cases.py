"""Random call sequences over the whole carver API and their reference.

program(seed) draws a JSON-able program -- the image, the configuration and 4 to 10 ops -- with the CPU oracle alone.  Shadow is the
reference runner: an oracle carver (oracle/lqr_oracle.c, which tests/test_oracle_later_calls.py pins to the genuine liblqr) plus
Python bookkeeping, the image shown at the last flat point and what happened since; for every op it says what the engine must
return and show.  Runner executes the same op on the engine (at 8 bits, or on a lifted twin of the image), with guard bytes around
every host buffer and sentinel elements around every device tensor it hands in.  run(api, program) walks both and compares after
EVERY op: return value, getters, scan_by_row, lqrx_carver_size_range, the image, the dumped map, the attached carver's image, the op's
own output (bits for floats).

The ops, what referees each, and when the generator may draw it (state: what the carver is like BEFORE the op):

  kind            call                                                       reference                              precondition
  resize          lqr_carver_resize, both directions, shrinking, back         the oracle, resized direction by        initialised (a carver that holds a loaded map and
                  inside the map, beyond it, enlarging past enl_step          direction and step by step (below)      is not initialised: sizes of the map only)
  flatten         lqr_carver_flatten                                          the oracle                              --
  set_energy      lqr_carver_set_energy_function_builtin (0 .. 6)             the oracle                              --
  bias_rgb        lqr_carver_bias_add_rgb_area, offsets that clip             the oracle                              initialised (lqr.h's form refuses others)
  rig_rgb         lqr_carver_rigmask_add_rgb_area                             the oracle                              initialised
  bias_f          lqr_carver_bias_add_area / _bias_add on a gdouble plane     the oracle                              --
  bias_dev        lqrx_carver_bias_add_area_device, 32F or 64F tensor         the oracle's gdouble form of the        --
                                                                              widened values
  rig_f, rig_dev  lqr_carver_rigmask_add_area, ..._area_device                as bias_f, bias_dev                     initialised
  bias_xy, rig_xy runs of lqr_carver_bias_add_xy / _rigmask_add_xy            the oracle                              rig_xy: initialised
  bias_clear, rig_clear                                                       the oracle                              --
  energy          lqr_carver_get_true_energy / _get_energy / _get_energy_     the oracle's true plane, then           --
  energy_dev      image; lqrx_carver_get_energy_device / _image_device        energy_cases.normalised / picture
  init            lqr_carver_init on a carver created (or reopened) without   the oracle                              not initialised
  read_sizes      lqrx_carver_read_sizes at up to 4 sizes of the range        sizes_cases.fast_model(image at the     --
  read_sizes_dev  lqrx_carver_read_sizes_device                               last flat point, the oracle's map)
  forward_map     lqrx_carver_forward_map                                     forward_cases.forward_map of            --
  forward_map_dev lqrx_carver_forward_map_device                              forward_cases.intensity of the image
                                                                              shown and the oracle's bias plane; the
                                                                              oracle is flattened when it is not flat
  planes          lqrx_carver_get_bias, lqrx_carver_get_rigmask (an op of its   the oracle's planes                     flat
                  own: a read-out after every op would flush the queued _xy
                  values before the op that has to)
  reopen          the ENGINE carver is replaced by a new one of the image     the oracle, which goes on as it was     initialised, not flat, no mask since creation;
                  at the last flat point that loads the oracle's map          (its enl_step becomes 2.0, as a load    rigidity 0 and switch_freq 0 (below)
                  (lqr_vmap_load; "device": lqrx_vmap_load_device; "init":    sets it)
                  lqr_carver_init after the load) and resized to the size
                  shown; "noinit" serves only the map's sizes until an init
  load_forward    lqrx_carver_load_forward                                    the model: vmap_cases.model of the      rigidity 0, switch_freq 0, no mask since creation
  resize_forward  lqrx_carver_resize_forward                                  image shown under forward_cases' map;
                                                                              afterwards resize inside the map,
                                                                              read_sizes and flatten only; at a
                                                                              flatten the shadow starts a new oracle
                                                                              carver of the image shown
  bad_init, bad_resize   a second lqr_carver_init; a width of 0               LQR_ERROR from both; the program ends   last op of a share of programs

The image at the last flat point.  A resize flattens by itself when it changes direction and between the steps of an enlargement past
enl_step.  Shadow therefore resizes the oracle one direction at a time (lqr_carver_resize(w1, h1) IS resize_dir(w1) then
resize_dir(h1), and a direction whose size does not change does nothing) and an enlargement one step at a time (the next call's first
iteration is the flatten the one call would have made), and takes the image shown before each of them.  tests/test_sequences.py
checks that bookkeeping on every op of every program: vmap_cases.model(that image, the oracle's map, the size) is the oracle's image.

Narrower than the headers say, and why (NOTES/sequence-tests.md):
  * reopen and the forward loads want switch_freq 0: which side wins ties (liblqr's leftright) is carver state that survives
    flattening, a new carver starts on the left, and neither lqr_vmap.h item 5 nor lqr_forward.h says so;
  * a new session is drawn with 3 .. 40 seams only where the side can lose 3 and stay at 5; a smaller carver is enlarged or carved
    the other way instead (resizes inside a map, and the depth of a forward map, may be any number);
  * they want rigidity 0: liblqr rescales its rigidity table at every transposition (float), a new carver computes it afresh.

Left out: lqr_carver_cancel (tests/test_control_gpu.py), allocation failures and fault injection, and every input on which a header
says the engine does not follow liblqr: read-outs and bias forms on attached carvers, frames one pixel wide (no side below 5), depths
outside the enum, LQR_CUSTOM_IMAGE, non-finite pixels, _xy calls outside the image, lqr_carver_rigmask_add / _add_rgb (the whole-size
forms) on a carver that may not be flat, second loads and refused resizes of lqr_vmap.h items 2 and 3.

Lifted twins.  A program in which no op asks for a size above the reference size (in either direction) creates no pixel by averaging; it is also run on the 16I
image v * 257 and the 64F image v / 255.0: the same return values, getters and maps, pixels the 8-bit ones lifted, energies bit-equal.
(read_sizes may ask such a carver for a size above its reference size; those pixels are averages, which each depth rounds its own way,
so for the twins the read_sizes reference is the same model applied to the lifted image at the last flat point.)
"""
import ctypes as C
import json

import numpy as np

import coldepth_cases as CD
import energy_cases as EC
import forward_cases as FC
import imgtype_cases as IT
import lqr_ctypes as L
import sizes_cases as SC
import vmap_cases as VC

GUARD = 64                      # bytes of 0xA5 before and behind every host buffer handed to the engine
PAD = 3                         # sentinel elements before and behind every device tensor (odd: the slice is not vector-aligned)
CLASSES = ("flat", "shrunk", "regrown", "enlarged", "transposed-flat", "transposed-not-flat")
LIFT_CLASSES = ("flat", "shrunk", "regrown", "transposed-flat", "transposed-not-flat")
FLAGS = ("init", "bias", "rig", "aux")
DTYPES = CD.DTYPES

# kind -> what the state must be: init (True: initialised, False: not, None: either), clean (no mask since creation), plain
# (rigidity 0 and switch_freq 0), notflat (holds a map), classes the kind can be drawn in
_FLAT = ("flat", "transposed-flat")
OPS = {
    "resize": dict(init=True), "flatten": dict(), "set_energy": dict(),
    "bias_rgb": dict(init=True), "rig_rgb": dict(init=True), "bias_f": dict(), "bias_dev": dict(), "rig_f": dict(init=True),
    "rig_dev": dict(init=True), "bias_xy": dict(), "rig_xy": dict(init=True), "bias_clear": dict(), "rig_clear": dict(),
    "energy": dict(), "energy_dev": dict(), "init": dict(init=False), "read_sizes": dict(), "read_sizes_dev": dict(),
    "forward_map": dict(), "forward_map_dev": dict(), "planes": dict(flat=True),
    "reopen": dict(init=True, clean=True, notflat=True, plain=True), "load_forward": dict(clean=True, plain=True),
    "resize_forward": dict(clean=True, plain=True),
}
for _k, _v in OPS.items():
    _v.setdefault("init", None)
    _v["classes"] = tuple(c for c in CLASSES if not (_v.get("flat") and c not in _FLAT) and not (_v.get("notflat") and c in _FLAT))
MODEL_KINDS = ("resize", "flatten", "read_sizes", "read_sizes_dev")         # what may follow a forward load
NOINIT_KINDS = ("resize", "read_sizes", "read_sizes_dev", "init")           # what may follow reopen "noinit"
TARGETS = [(k, c) for k in OPS for c in OPS[k]["classes"]]


ROUNDS = 10             # seeds per (op kind, state class) target; round r of a target fixes the four flags (flag_plan)


def can_be_uninitialised(kind, cls):
    """a carver that lqr_carver_init has not seen is flat (new; transposed by a read-out), or it holds a map it was given: the
    classes that are not flat are reached without init only through a reopen, after which NOINIT_KINDS alone may be drawn"""
    if OPS[kind]["init"]:
        return False
    return cls in _FLAT or kind in NOINIT_KINDS


def feasible(kind, cls, flag, value):
    """can op `kind` meet a carver of class `cls` whose `flag` is `value`?  What cannot exist, and why:
      * a class or a flag value the kind's own precondition excludes (OPS, flag_values);
      * not initialised and not flat, except before NOINIT_KINDS (can_be_uninitialised);
      * `init` on a carver that is not flat with a bias: that carver was reopened, and a reopen wants no mask since creation
        (a rigidity mask never meets `init`: it needs the initialised carver).
    A few meetings outside this rule do happen (a resize or a flatten of an uninitialised carver that holds a forward map or was
    reopened); they are counted and printed, and not required."""
    if cls not in OPS[kind]["classes"] or value not in flag_values(kind, flag):
        return False
    if flag == "init" and not value:
        return can_be_uninitialised(kind, cls)
    if kind == "init" and cls not in _FLAT and flag in ("bias", "rig") and value:
        return False
    return True


def flag_plan(kind, cls, r):
    """the flags round r of target (kind, cls) sets up, so that over ROUNDS rounds every feasible (kind, cls, flag, value) is met at
    least 5 times: uninitialised in rounds 0, 1, 4, 5, 8 and a rigidity mask in 2, 3, 6, 7, 9 (the two exclude each other), a bias
    in the odd rounds, an attached carver in 4 .. 8.  Where a carver is uninitialised AND not flat it came through a reopen and has
    no mask, so there the other five rounds carry both masks."""
    v = OPS[kind]
    uninit = v["init"] is False or (can_be_uninitialised(kind, cls) and r in (0, 1, 4, 5, 8))
    bias, rig = r % 2 == 1, r in (2, 3, 6, 7, 9)
    if v["init"] is None and cls not in _FLAT and kind in NOINIT_KINDS:
        bias = rig = not uninit
    if uninit and cls not in _FLAT:
        bias = rig = False
    if uninit or v.get("clean"):
        rig = False
    if v.get("clean"):
        bias = False
    return dict(init=not uninit, bias=bias, rig=rig, aux=r in (4, 5, 6, 7, 8))


def flag_values(kind, flag):
    """the values of a state flag under which the kind's precondition lets it be drawn"""
    v = OPS[kind]
    if flag == "init":
        return (True, False) if v["init"] is None else (v["init"],)
    if flag in ("bias", "rig") and v.get("clean"):
        return (False,)
    if flag == "rig" and kind == "init":
        return (False,)                         # a rigidity mask needs the initialised carver
    return (True, False)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_image(prog):
    i = prog["image"]
    return CD.base_image(np.random.default_rng([i["seed"], 1]), i["w"], i["h"], i["ch"])


def make_aux(prog):
    i = prog["image"]
    return CD.base_image(np.random.default_rng([i["seed"], 2]), i["w"], i["h"], 3)


def lift(img, depth):
    """coldepth_cases' lift rule: the 16I image v * 257, the 64F image v / 255.0 read the same doubles as the 8-bit v"""
    if depth == 0:
        return np.ascontiguousarray(img)
    if depth == 1:
        return img.astype(np.uint16) * np.uint16(257)
    assert depth == 3
    return img.astype(np.float64) / 255.0


def mask_u8(seed, w, h, ch):
    return np.random.default_rng([seed, 3]).integers(0, 256, (h, w, ch)).astype(np.uint8)


def mask_f(seed, w, h, dtype):
    """values in [-1, 2) of the dtype the caller holds them in ("f8" host gdouble / 64F tensor, "f4" 32F tensor)"""
    return np.random.default_rng([seed, 4]).uniform(-1.0, 2.0, (h, w)).astype(dtype)


def xy_run(seed, W, H, n):
    rng = np.random.default_rng([seed, 5, W, H])
    pix = rng.integers(0, W * H, n)
    val = rng.integers(-8, 17, n).astype(np.float64) / 4.0
    return [(int(p % W), int(p // W), float(v)) for p, v in zip(pix, val)]


def delta_max(enl_step, ref):
    d = int(np.float32(np.float32(enl_step) - np.float32(1)) * np.float32(ref)) - 1
    return max(d, 1)


def size_range(g):
    """lqrx_carver_size_range from the getters (include/lqr_sizes.h)"""
    o = g["orientation"]
    ref = g["ref_height"] if o else g["ref_width"]
    return [o, ref - g["depth"], ref + min(g["depth"], delta_max(g["enl_step"], ref))]


def classify(g):
    o, d = g["orientation"], g["depth"]
    if d == 0:
        return "transposed-flat" if o else "flat"
    if o:
        return "transposed-not-flat"
    if g["width"] > g["ref_width"]:
        return "enlarged"
    return "shrunk" if g["width"] == g["ref_width"] - d else "regrown"


def is_flat(g):
    return g["depth"] == 0 and g["width"] == g["ref_width"] and g["height"] == g["ref_height"]


def ok_ret(ret):
    return ret is None or ret == 1 or (isinstance(ret, list) and all(v == 1 for v, _ in ret))


def _summary(rets):
    return [[int(v), int(rets.count(v))] for v in sorted(set(rets))]


def energy_shape(op, w, h):
    """(dtype, shape) of what an energy op writes: ["energy" | "energy_dev", form, o, depth, type]"""
    form, depth, image_type = op[1], op[3], op[4]
    if form == 2:
        return np.dtype(EC.DTYPES[depth]), (h, w, IT.TYPE_CHANNELS[image_type])
    return np.dtype(np.float32), (h, w)


# ---- the shadow ---------------------------------------------------------------------------------------------------------------
class Shadow:
    def __init__(self, prog):
        self.prog, self.cfg = prog, prog["config"]
        self.api = L.bind_energy(L.bind_masks(L.oracle_api()))
        self.ch = prog["image"]["ch"]
        self.nrg = self.cfg["nrg"]
        self.active = not self.cfg["late_init"]         # what the ENGINE carver is (a reopen without init parts the two)
        self.masked = self.has_bias = self.has_rig = False
        self.mode = "oracle"
        self.enlarged_ever = False
        self.c = self.aux = None
        self._new_oracle(make_image(prog), make_aux(prog) if self.cfg["aux"] else None, self.active, self.cfg["enl_step"], 0)

    def _new_oracle(self, img, aux_img, active, enl_step, orientation):
        if self.c is not None:
            self.c.destroy()
        cfg = self.cfg
        self.c = L.OracleCarver(self.api, img, init=active, delta_x=cfg["delta"], rigidity=cfg["rigidity"])
        self.aux = self.c.attach(aux_img) if aux_img is not None else None
        self.c.configure(nrg_func=self.nrg, res_order=cfg["res_order"], switch_freq=cfg["switch_freq"], enl_step=enl_step)
        if orientation:                                 # a flat carver that lies the other way: a read-out leaves it so
            h, w = img.shape[:2]
            assert self.c.energy_call(0, 1, nbytes=4 * w * h)[0] == 1
        self.base, self.aux_base = np.ascontiguousarray(img), aux_img
        self.oracle_active = active

    def close(self):
        if self.c is not None:
            self.c.destroy()
            self.c = None

    # -- what the carver shows -----------------------------------------------------------------------------------------------
    def getters(self):
        if self.mode == "model":
            m = self.m
            return dict(width=m["w"], height=m["h"], channels=self.ch, ref_width=m["rw"], ref_height=m["rh"], orientation=m["map"]["orientation"],
                        depth=m["map"]["depth"], enl_step=2.0)
        g = self.c.getters()
        g["enl_step"] = float(g["enl_step"])
        return g

    def vmap(self):
        return self.m["map"] if self.mode == "model" else self.c.vmap_dump()

    def _size(self, g):
        return g["height"] if g["orientation"] else g["width"]

    def image(self):
        if self.mode == "model":
            return SC.fast_model(self.base, self.m["map"], self._size(self.getters()))
        return self.c.read_scanlines()[0]

    def aux_image(self):
        if self.aux_base is None:
            return None
        if self.mode == "model":
            return SC.fast_model(self.aux_base, self.m["map"], self._size(self.getters()))
        return self.aux.read_scanlines()[0]

    def state(self):
        g = self.getters()
        # loadable: lqr_vmap.h item 6 -- a carver carved down to one column dumps liblqr's finish mark, a level above the depth
        return dict(g=g, cls=classify(g), init=self.active, bias=self.has_bias, rig=self.has_rig, aux=self.aux_base is not None,
                    masked=self.masked, mode=self.mode, nrg=self.nrg, range=size_range(g), loadable=g["depth"] > 0 and int(self.vmap()["data"].max()) <= g["depth"])

    def observe(self, ret, out=(), state=None):
        g = self.getters()
        return dict(ret=ret, getters=g, by_row=not g["orientation"], range=size_range(g), image=self.image(), vmap=self.vmap(),
                    aux=self.aux_image(), out=list(out), state=state, base=self.base, aux_base=self.aux_base, mode=self.mode)

    def _rebase(self):
        """after anything on the oracle: a flat carver's image is the image at the last flat point"""
        if self.mode == "oracle" and is_flat(self.getters()):
            self.base = self.c.read_scanlines()[0]
            if self.aux is not None:
                self.aux_base = self.aux.read_scanlines()[0]

    def _take_shown(self):
        self.base = self.c.read_scanlines()[0]
        if self.aux is not None:
            self.aux_base = self.aux.read_scanlines()[0]

    # -- the ops -------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        state = self.state()
        kind = op[0]
        ret, out = getattr(self, "_" + kind)(*op[1:])
        self._rebase()
        obs = self.observe(ret, out, state)
        obs["kind"] = kind
        if kind == "reopen":
            obs["reopen"] = self.reopen
        g = obs["getters"]
        if g["width"] > g["ref_width"] or g["height"] > g["ref_height"]:
            self.enlarged_ever = True
        return obs

    def _resize(self, w1, h1):
        if self.mode == "model":
            m = self.m
            o = m["map"]["orientation"]
            assert (w1 == m["w"]) if o else (h1 == m["h"]), "a loaded map serves its own direction"
            lo, hi = size_range(self.getters())[1:]
            assert lo <= (h1 if o else w1) <= hi
            m["w"], m["h"] = w1, h1
            return 1, []
        if w1 < 1 or h1 < 1:
            return self.c.resize(w1, h1), []
        for d in ((0, 1) if self.cfg["res_order"] == 0 else (1, 0)):
            while True:
                g = self.getters()
                cur, target = (g["height"], h1) if d else (g["width"], w1)
                if cur == target:
                    break
                if g["orientation"] != d:               # the carver is flattened and transposed: what it shows is the new base
                    self._take_shown()
                    ref = cur
                else:
                    ref = g["ref_height"] if d else g["ref_width"]
                    if target > cur == ref + delta_max(g["enl_step"], ref):
                        self._take_shown()              # an enlargement goes on: the call's first step is the flatten
                        ref = cur
                step = min(target, ref + delta_max(g["enl_step"], ref))
                ret = self.c.resize(g["width"] if d else step, step if d else g["height"])
                if ret != 1:
                    return ret, []
        return 1, []

    def _flatten(self):
        if self.mode == "model":
            g = self.getters()
            shown, aux_shown = self.image(), self.aux_image()
            self.mode = "oracle"
            self._new_oracle(shown, aux_shown, self.active, 2.0, g["orientation"])
            return 1, []
        return self.c.flatten(), []

    def _set_energy(self, nrg):
        self.nrg = nrg
        return self.c.set_energy(nrg), []

    def _bias_rgb(self, seed, mw, mh, mch, factor, xo, yo):
        self.masked = True
        self.has_bias = self.has_bias or factor != 0
        return self.c.bias_add(mask_u8(seed, mw, mh, mch), factor, xo, yo), []

    def _rig_rgb(self, seed, mw, mh, mch, xo, yo):
        self.masked = self.has_rig = True
        return self.c.rigmask_add(mask_u8(seed, mw, mh, mch), xo, yo), []

    def _bias_f(self, seed, mw, mh, factor, xo, yo, dtype="f8"):
        self.masked = True
        self.has_bias = self.has_bias or factor != 0
        return self.c.bias_add_f(mask_f(seed, mw, mh, dtype).astype(np.float64), factor, xo, yo), []

    def _bias_dev(self, seed, mw, mh, factor, xo, yo, dtype):
        return self._bias_f(seed, mw, mh, factor, xo, yo, dtype)

    def _rig_f(self, seed, mw, mh, xo, yo, dtype="f8"):
        self.masked = self.has_rig = True
        return self.c.rigmask_add_f(mask_f(seed, mw, mh, dtype).astype(np.float64), xo, yo), []

    def _rig_dev(self, seed, mw, mh, xo, yo, dtype):
        return self._rig_f(seed, mw, mh, xo, yo, dtype)

    def _xy(self, which, seed, n):
        g = self.getters()
        run = xy_run(seed, g["width"], g["height"], n)
        self.masked = True
        if which == "bias":
            self.has_bias = self.has_bias or any(v != 0 for _, _, v in run)
            return _summary(self.c.bias_add_xy(run)), []
        self.has_rig = True
        return _summary(self.c.rigmask_add_xy(run)), []

    def _bias_xy(self, seed, n):
        return self._xy("bias", seed, n)

    def _rig_xy(self, seed, n):
        return self._xy("rig", seed, n)

    def _bias_clear(self):
        self.has_bias = False
        self.c.bias_clear()
        return None, []

    def _rig_clear(self):
        self.has_rig = False
        self.c.rigmask_clear()
        return None, []

    def _energy(self, form, o, depth, image_type):
        g = self.getters()
        dt, shape = energy_shape(["energy", form, o, depth, image_type], g["width"], g["height"])
        n = int(np.prod(shape)) * dt.itemsize
        ret, buf = self.c.energy_call(form, o, depth, image_type, nbytes=n, guard=0)
        return ret, [buf.view(dt).reshape(shape)]

    _energy_dev = _energy

    def _init(self):
        if not self.active and self.oracle_active:      # (a reopen without init: only the engine's carver is new)
            self.active = True
            return 1, []
        ret = self.c.init(self.cfg["delta"], self.cfg["rigidity"])
        self.active = self.oracle_active = self.active or ret == 1
        return ret, []

    def _read_sizes(self, sizes):
        return 1, [SC.fast_model(self.base, self.vmap(), s) for s in sizes]

    _read_sizes_dev = _read_sizes

    def forward_model(self, d, o):
        """the model's map of what the carver shows; the oracle is flattened when the engine flattens (lqr_forward.h: a carver that
        is not flat)"""
        if not is_flat(self.getters()):
            assert self.c.flatten() == 1
            self._rebase()
        img = self.c.read_scanlines()[0]
        I = FC.intensity(img, 0, IT.TypeState(self.ch), 3 <= self.nrg <= 5)
        return FC.forward_map(I, self.c.get_bias(), d, o)

    def _forward_map(self, d, o):
        m = self.forward_model(d, o)
        return 1, [m["data"], np.array([m["depth"], m["orientation"]])]

    _forward_map_dev = _forward_map

    def _planes(self):
        return None, [self.c.get_bias(), self.c.get_rigmask()]

    def _reopen(self, variant):
        """the inputs the engine's new carver gets are left in self.reopen"""
        g = self.getters()
        self.reopen = dict(base=self.base, aux=self.aux_base, map=self.c.vmap_dump(), size=(g["width"], g["height"]))
        assert self.api.lqr_carver_set_enl_step(self.c.p, 2.0) == 1
        self.active = variant == "init"
        return 1, []

    def _load_forward(self, d, o):
        if self.mode == "model":                        # what is shown becomes a flat carver again
            self._flatten()
        m = self.forward_model(d, o)
        self._take_shown()
        g = self.getters()
        self.mode = "model"
        self.m = dict(map=m, w=g["width"], h=g["height"], rw=g["width"], rh=g["height"])
        return 1, []

    def _resize_forward(self, w1, h1):
        for d in ((0, 1) if self.cfg["res_order"] == 0 else (1, 0)):
            g = self.getters()
            change = (h1 - g["height"]) if d else (w1 - g["width"])
            if change:
                self._load_forward(abs(change), d)
                self._resize(g["width"] if d else w1, h1 if d else g["height"])
        return 1, []

    def _bad_init(self):
        return self.c.init(self.cfg["delta"], self.cfg["rigidity"]), []

    def _bad_resize(self, w1, h1):
        return self.c.resize(w1, h1), []


# ---- the engine's side ----------------------------------------------------------------------------------------------------------
def _guarded(arr):
    """(the whole buffer, a view of arr's shape inside it) with GUARD bytes of 0xA5 on either side"""
    arr = np.ascontiguousarray(arr)
    big = np.full(arr.nbytes + 2 * GUARD, 0xa5, np.uint8)
    view = big[GUARD:GUARD + arr.nbytes].view(arr.dtype).reshape(arr.shape)
    view[...] = arr
    return big, view


def _guards_intact(big):
    return bool((big[:GUARD] == 0xa5).all() and (big[-GUARD:] == 0xa5).all())


class Runner:
    """one program on the engine; depth: 0, or the colour depth of a lifted twin (1: 16I, 3: 64F)"""

    def __init__(self, api, prog, depth=0):
        self.api = L.bind_forward(L.bind_sizes(L.bind_energy(L.bind_masks(L.bind_vmap(L.bind_coldepth(api))))))
        self.prog, self.cfg, self.depth = prog, prog["config"], depth
        self.nrg = self.cfg["nrg"]
        self.c = None
        self._new(make_image(prog), make_aux(prog) if self.cfg["aux"] else None, not self.cfg["late_init"])

    def _new(self, img, aux_img, init):
        if self.c is not None:
            self.c.destroy()
        cfg = self.cfg
        self.c = L.Carver.from_ext(self.api, lift(img, self.depth), self.depth, init=init, delta_x=cfg["delta"], rigidity=cfg["rigidity"])
        self.aux = self.c.attach_ext(aux_img, 0) if aux_img is not None else None
        self.c.configure(nrg_func=self.nrg, res_order=cfg["res_order"], switch_freq=cfg["switch_freq"], enl_step=cfg["enl_step"])

    def close(self):
        if self.c is not None:
            self.c.destroy()
            self.c = None

    def observe(self, ret, out, intact):
        c = self.c
        g = c.getters()
        g["enl_step"] = float(g["enl_step"])
        return dict(ret=ret, getters=g, by_row=bool(self.api.lqr_carver_scan_by_row(c.p)), range=list(c.size_range()),
                    image=c.scan_line_ext()[0], vmap=c.vmap_dump(), aux=self.aux.scan_line_ext()[0] if self.aux is not None else None,
                    out=list(out), intact=intact, col_depth=self.api.lqr_carver_get_col_depth(c.p))

    def apply(self, op, want):
        """want: the shadow's observation of the op (a reopen takes its inputs from it)"""
        self.intact = True
        ret, out = getattr(self, "_" + op[0])(want, *op[1:])
        return self.observe(ret, out, self.intact)

    def _check(self, big, view=None, want=None):
        if not _guards_intact(big) or (want is not None and not np.array_equal(CD.bits(view), CD.bits(want))):
            self.intact = False                         # (an input the call wrote to counts as a broken guard)

    # -- device tensors with sentinel elements on either side
    def _tensor(self, arr):
        import torch
        arr = np.ascontiguousarray(arr)
        store = {2: np.int16, 1: np.uint8}.get(arr.dtype.itemsize if arr.dtype.kind in "ui" else 0, arr.dtype)
        flat = np.concatenate([np.full(PAD, 0x5a, store), arr.view(store).ravel(), np.full(PAD, 0x5a, store)])
        whole = torch.from_numpy(flat).cuda()
        return whole, whole[PAD:PAD + arr.size].view(*arr.shape), flat

    def _tensor_back(self, whole, flat, n, dtype, shape, written):
        """the middle of the tensor as a numpy array; the sentinels (and, for an input, the middle) must be as they were"""
        back = whole.cpu().numpy()
        if not (np.array_equal(back[:PAD], flat[:PAD]) and np.array_equal(back[PAD + n:], flat[PAD + n:])):
            self.intact = False
        if not written and not np.array_equal(back.view(np.uint8), flat.view(np.uint8)):
            self.intact = False
        return back[PAD:PAD + n].view(dtype).reshape(shape)

    # -- the ops
    def _resize(self, sh, w1, h1):
        return self.c.resize(w1, h1), []

    _bad_resize = _resize

    def _flatten(self, sh):
        return self.c.flatten(), []

    def _set_energy(self, sh, nrg):
        self.nrg = nrg
        return self.c.set_energy(nrg), []

    def _host_mask(self, arr, call):
        big, view = _guarded(arr)
        ret = call(view)
        self._check(big, view, arr)
        return ret, []

    def _bias_rgb(self, sh, seed, mw, mh, mch, factor, xo, yo):
        return self._host_mask(mask_u8(seed, mw, mh, mch), lambda m: self.c.bias_add(m, factor, xo, yo))

    def _rig_rgb(self, sh, seed, mw, mh, mch, xo, yo):
        return self._host_mask(mask_u8(seed, mw, mh, mch), lambda m: self.c.rigmask_add(m, xo, yo))

    def _bias_f(self, sh, seed, mw, mh, factor, xo, yo):
        return self._host_mask(mask_f(seed, mw, mh, "f8"), lambda m: self.c.bias_add_f(m, factor, xo, yo))

    def _rig_f(self, sh, seed, mw, mh, xo, yo):
        return self._host_mask(mask_f(seed, mw, mh, "f8"), lambda m: self.c.rigmask_add_f(m, xo, yo))

    def _dev_mask(self, arr, call):
        whole, t, flat = self._tensor(arr)
        ret = call(t)
        self._tensor_back(whole, flat, arr.size, arr.dtype, arr.shape, written=False)
        return ret, []

    def _bias_dev(self, sh, seed, mw, mh, factor, xo, yo, dtype):
        return self._dev_mask(mask_f(seed, mw, mh, dtype), lambda t: self.c.bias_add_device(t, factor, 0 if xo is None else xo, 0 if yo is None else yo))

    def _rig_dev(self, sh, seed, mw, mh, xo, yo, dtype):
        return self._dev_mask(mask_f(seed, mw, mh, dtype), lambda t: self.c.rigmask_add_device(t, xo, yo))

    def _bias_xy(self, sh, seed, n):
        g = self.c.getters()
        return _summary(self.c.bias_add_xy(xy_run(seed, g["width"], g["height"], n))), []

    def _rig_xy(self, sh, seed, n):
        g = self.c.getters()
        return _summary(self.c.rigmask_add_xy(xy_run(seed, g["width"], g["height"], n))), []

    def _bias_clear(self, sh):
        self.c.bias_clear()
        return None, []

    def _rig_clear(self, sh):
        self.c.rigmask_clear()
        return None, []

    def _energy(self, sh, form, o, depth, image_type):
        g = self.c.getters()
        dt, shape = energy_shape(["energy", form, o, depth, image_type], g["width"], g["height"])
        big, view = _guarded(np.zeros(shape, dt))
        a, p = self.api, self.c.p
        if form == 2:
            ret = a.lqr_carver_get_energy_image(p, view.ctypes.data, o, depth, image_type)
        else:
            ret = (a.lqr_carver_get_energy if form else a.lqr_carver_get_true_energy)(p, view.ctypes.data, o)
        self._check(big)
        return ret, [view.copy()]

    def _energy_dev(self, sh, form, o, depth, image_type):
        import torch
        g = self.c.getters()
        dt, shape = energy_shape(["energy", form, o, depth, image_type], g["width"], g["height"])
        whole, t, flat = self._tensor(np.zeros(shape, dt))
        torch.cuda.current_stream().synchronize()
        a, p = self.api, self.c.p
        if form == 2:
            ret = a.lqrx_carver_get_energy_image_device(p, t.data_ptr(), o, depth, image_type)
        else:
            ret = a.lqrx_carver_get_energy_device(p, t.data_ptr(), o, 1 if form else 0)
        return ret, [self._tensor_back(whole, flat, int(np.prod(shape)), dt, shape, written=True)]

    def _init(self, sh):
        return self.c.init(self.cfg["delta"], self.cfg["rigidity"]), []

    _bad_init = _init

    def _sizes_shapes(self, sizes):
        return [self.c._sizes_shape(s) for s in sizes], np.dtype(DTYPES[self.depth])

    def _read_sizes(self, sh, sizes):
        shapes, dt = self._sizes_shapes(sizes)
        bufs = [_guarded(np.zeros(s, dt)) for s in shapes]
        arr = (C.c_int * len(sizes))(*sizes)
        ptrs = (C.c_void_p * len(sizes))(*[v.ctypes.data for _, v in bufs])
        ret = self.api.lqrx_carver_read_sizes(self.c.p, arr, len(sizes), ptrs)
        for big, _ in bufs:
            self._check(big)
        return ret, [v.copy() for _, v in bufs]

    def _read_sizes_dev(self, sh, sizes):
        import torch
        shapes, dt = self._sizes_shapes(sizes)
        ts = [self._tensor(np.zeros(s, dt)) for s in shapes]
        torch.cuda.current_stream().synchronize()
        arr = (C.c_int * len(sizes))(*sizes)
        ptrs = (C.c_void_p * len(sizes))(*[t.data_ptr() for _, t, _ in ts])
        ret = self.api.lqrx_carver_read_sizes_device(self.c.p, arr, len(sizes), ptrs)
        return ret, [self._tensor_back(whole, flat, int(np.prod(s)), dt, s, written=True) for (whole, _, flat), s in zip(ts, shapes)]

    def _forward_map(self, sh, d, o):
        m = self.c.forward_map(d, o)
        if m is None:
            return 0, []
        return 1, [m["data"], np.array([m["depth"], m["orientation"]])]

    def _forward_map_dev(self, sh, d, o):
        g = self.c.getters()
        shape = (g["height"], g["width"])
        whole, t, flat = self._tensor(np.full(shape, -1, np.int32))
        ret = self.c.forward_map_device(t, d, o)
        return ret, [self._tensor_back(whole, flat, shape[0] * shape[1], np.int32, shape, written=True), np.array([d, o])]

    def _planes(self, sh):
        g = self.c.getters()
        out = []
        for fn in (self.api.lqrx_carver_get_bias, self.api.lqrx_carver_get_rigmask):
            big, view = _guarded(np.zeros((g["height"], g["width"]), np.float32))
            assert fn(self.c.p, view.ctypes.data) == 1
            self._check(big)
            out.append(view.copy())
        return None, out

    def _reopen(self, sh, variant):
        r = sh["reopen"]
        self._new(r["base"], r["aux"], False)
        m = r["map"]
        if variant == "device":
            whole, t, flat = self._tensor(np.ascontiguousarray(m["data"], np.int32))
            ret = self.c.vmap_load_device(t, m["depth"], m["orientation"])
            self._tensor_back(whole, flat, m["data"].size, np.int32, m["data"].shape, written=False)
        else:
            ret = self.c.vmap_load(m)
        if ret == 1 and variant == "init":
            ret = self.c.init(self.cfg["delta"], self.cfg["rigidity"])
        if ret == 1:
            ret = self.c.resize(*r["size"])
        return ret, []

    def _load_forward(self, sh, d, o):
        return self.c.load_forward(d, o), []

    def _resize_forward(self, sh, w1, h1):
        return self.c.resize_forward(w1, h1), []


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(CD.bits(a), CD.bits(b))


def differences(want, got, depth=0):
    """what of an op's observation differs (an empty list: nothing); images are the 8-bit ones lifted to `depth`"""
    bad = []
    if want["ret"] != got["ret"]:
        return ["the return value differs: %r, the reference %r" % (got["ret"], want["ret"])]
    if not ok_ret(want["ret"]):
        return bad                                      # both refused: the program ends here
    for k in ("getters", "by_row", "range"):
        if want[k] != got[k]:
            bad.append("%s differs: %r, the reference %r" % (k, got[k], want[k]))
    if got["col_depth"] != depth:
        bad.append("col_depth differs: %r" % got["col_depth"])
    if not got["intact"]:
        bad.append("guard bytes or sentinel elements around a buffer differ from what was put there, or an input buffer was written")
    if not _same(lift(want["image"], depth), got["image"]):
        bad.append("the image differs")
    wv, gv = want["vmap"], got["vmap"]
    if (wv["depth"], wv["orientation"]) != (gv["depth"], gv["orientation"]) or not _same(np.asarray(wv["data"], np.int32), np.asarray(gv["data"], np.int32)):
        bad.append("the dumped map differs")
    if (want["aux"] is None) != (got["aux"] is None) or (want["aux"] is not None and not _same(want["aux"], got["aux"])):
        bad.append("the attached carver's image differs")
    if len(want["out"]) != len(got["out"]):
        bad.append("the number of outputs differs: %d, the reference %d" % (len(got["out"]), len(want["out"])))
    for i, (a, b) in enumerate(zip(want["out"], got["out"])):
        if not _same(lift(a, depth) if want.get("lift_out") else a, b):
            bad.append("output %d differs" % i)
    return bad


def run(api, prog, depth=0, seen=None):
    """the program on the engine `api` beside its shadow (api None: the shadow alone); returns the shadow's observations, one per op
    run, and raises AssertionError -- seed, op index, what differs, the program -- at the first op after which the two differ.
    seen: the shadow's observations from an earlier run of the same program, which then is not run again"""
    sh = Shadow(prog) if seen is None else None
    en = Runner(api, prog, depth) if api is not None else None
    out = []
    try:
        for i, op in enumerate(prog["ops"]):
            if sh is not None:
                want = sh.apply(op)
                want["lift_out"] = op[0] in ("read_sizes", "read_sizes_dev")
            else:
                want = seen[i]
            out.append(want)
            if en is not None:
                if depth and want["lift_out"]:          # a size above the reference size holds averages, which each depth rounds its own way
                    want = dict(want, lift_out=False, out=[SC.fast_model(lift(want["base"], depth), want["vmap"], s) for s in op[1]])
                bad = differences(want, en.apply(op, want), depth)
                assert not bad, "seed %d, op %d %s: %s\nprogram: %s" % (prog["seed"], i, json.dumps(op), "; ".join(bad), json.dumps(prog))
            if not ok_ret(want["ret"]):
                break
    finally:
        if sh is not None:
            sh.close()
        if en is not None:
            en.close()
    return out


SEEDS = list(range(ROUNDS * len(TARGETS)))


def run_checked(api, prog, depth=0, seen=None):
    """run(), and at the end of the program the engine's device pool has every block back and no session was rolled back"""
    lib = api.lib
    lib.lqrhip_debug_pool_live.restype, lib.lqrhip_debug_pool_live.argtypes = C.c_ulonglong, []
    lib.lqrhip_fault_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    st = (C.c_ulonglong * 8)()
    live = lib.lqrhip_debug_pool_live()
    assert lib.lqrhip_fault_stats(st, 1) == 0           # (reset)
    out = run(api, prog, depth, seen)
    what = "seed %d, depth %d\nprogram: %s" % (prog["seed"], depth, json.dumps(prog))
    assert lib.lqrhip_debug_pool_live() == live, "the device pool differs: blocks not given back, " + what
    assert lib.lqrhip_fault_stats(st, 0) == 0 and int(st[4]) == 0, "the roll-back counter differs from 0: a session was rolled back, " + what
    return out


def liftable(seen):
    """no op of the run asks for a size above the reference size the carver had BEFORE the op, in either direction: no pixel the
    carver ever holds was made by averaging (growing back inside the map only shows pixels again).  Comparing the size shown with
    the reference size AFTER every op is not enough: a resize that enlarges one direction and then changes the other flattens in
    between, and the enlarged image, averages included, is the reference size from then on."""
    def limit(o, side):                                 # (a forward load flattens first: what is shown is its reference size)
        return o["state"]["g"][side if o["kind"] in ("load_forward", "resize_forward") else "ref_" + side]
    return all(o["getters"][s] <= limit(o, s) and o["getters"][s] <= o["getters"]["ref_" + s] for o in seen for s in ("width", "height"))


# ---- the generator --------------------------------------------------------------------------------------------------------------
MIN_SEAMS, MIN_SIDE = 3, 5


def _room(size):
    """how many seams a side of `size` can lose (no side below MIN_SIDE); a session is drawn only where that is at least MIN_SEAMS"""
    return size - MIN_SIDE


def _seams(rng, room, least=MIN_SEAMS):
    """3 .. 40 seams, a share above 32 (the frozen lag of a small group), as far as `room` goes (callers ask only where room >= least)"""
    k = int(rng.integers(33, 41)) if rng.random() < 0.25 else int(rng.integers(3, 33))
    return max(least, min(k, room))


def _allowed(kind, st, cfg):
    v = OPS[kind]
    if st["mode"] == "model":
        return kind in MODEL_KINDS
    if not st["init"] and st["g"]["depth"] > 0:         # reopened without init: the map's sizes, or the init
        return kind in NOINIT_KINDS
    if v["init"] is not None and v["init"] != st["init"]:
        return False
    if v.get("clean") and st["masked"]:
        return False
    if v.get("plain") and (cfg["rigidity"] != 0 or cfg["switch_freq"] != 0):
        return False
    if v.get("notflat") and not st["loadable"]:
        return False
    if kind == "load_forward" and max(st["g"]["width"], st["g"]["height"]) <= MIN_SIDE:
        return False
    return st["cls"] in v["classes"]


def _resize_to(rng, st, cls=None):
    """a resize op from state st; cls: the class it should end in (None: anything an initialised carver may be asked)"""
    g = st["g"]
    w, h, o = g["width"], g["height"], g["orientation"]
    _, lo, hi = st["range"]
    ref = g["ref_height"] if o else g["ref_width"]
    along = lambda s: ["resize", w, s] if o else ["resize", s, h]               # noqa: E731  (the direction the carver lies in)
    across = lambda s: ["resize", s, h] if o else ["resize", w, s]              # noqa: E731
    cur, other = (h, w) if o else (w, h)
    restricted = st["mode"] == "model" or not st["init"]
    if cls is None:
        picks = ["inside"] if restricted else ["deeper", "deeper", "inside", "enlarge", "across", "across", "both", "beyond"]
        how = picks[int(rng.integers(0, len(picks)))]
        if how == "inside" and lo == hi:
            how = "inside" if restricted else "deeper"
        if how == "inside":
            return along(int(rng.integers(max(lo, min(MIN_SIDE, hi)), hi + 1)))        # (a map made by enlarging reaches below MIN_SIDE)
        if how == "deeper" and _room(lo) >= MIN_SEAMS:
            return along(lo - _seams(rng, _room(lo)))
        if how == "enlarge":
            return along(cur + 1 + int(rng.integers(0, delta_max(g["enl_step"], cur))))
        if how == "beyond":                             # past enl_step: more than one session, a flatten between them
            return along(cur + delta_max(g["enl_step"], cur) + int(rng.integers(1, 6)))
        if how == "both" and _room(cur) >= MIN_SEAMS and _room(other) >= MIN_SEAMS:
            return ["resize", w - _seams(rng, _room(w)), h - _seams(rng, _room(h))]
        return across(other - _seams(rng, _room(other))) if _room(other) >= MIN_SEAMS and rng.random() < 0.7 else across(other + 1 + int(rng.integers(0, 3)))
    # towards a class
    if cls == "shrunk":
        if o == 0:
            return along(lo - _seams(rng, _room(lo))) if _room(lo) >= MIN_SEAMS else along(lo)
        return across(other - _seams(rng, _room(other))) if _room(other) >= MIN_SEAMS else across(other + 1)
    if cls == "regrown":
        if o == 0 and g["depth"] > 0 and ref > lo:
            return along(int(rng.integers(lo + 1, ref + 1)))
        return _resize_to(rng, st, "shrunk")
    if cls == "enlarged":
        if o == 0:
            if hi > ref:
                return along(int(rng.integers(ref + 1, hi + 1)))
            return along(cur + 1 + int(rng.integers(0, min(40, delta_max(g["enl_step"], cur)))))
        return across(other + 1 + int(rng.integers(0, min(40, delta_max(g["enl_step"], other)))))
    if cls in ("transposed-not-flat", "transposed-flat"):
        if o == 1:
            return along(lo - _seams(rng, _room(lo))) if _room(lo) >= MIN_SEAMS else along(cur + 1)
        return across(other - _seams(rng, _room(other))) if _room(other) >= MIN_SEAMS and rng.random() < 0.8 else across(other + 1 + int(rng.integers(0, 3)))
    assert cls == "flat"
    return across(other - _seams(rng, _room(other))) if _room(other) >= MIN_SEAMS else across(other + 1)      # (from a transposed carver: back, then flatten)


def _towards(rng, st, cls):
    """one op that brings an initialised carver nearer to class cls, or None when it is there"""
    if st["cls"] == cls:
        return None
    if cls == "flat":
        return ["flatten"] if st["g"]["orientation"] == 0 else _resize_to(rng, st, "flat")
    if cls == "transposed-flat":
        return ["flatten"] if st["cls"] == "transposed-not-flat" else _resize_to(rng, st, cls)
    return _resize_to(rng, st, cls)


def _mask_args(rng, g):
    """a mask smaller or larger than the image at offsets that clip on any side"""
    W, H = g["width"], g["height"]
    mw, mh = int(rng.integers(max(1, W // 3), W + 12)), int(rng.integers(max(1, H // 3), H + 6))
    return mw, mh, int(rng.integers(-mw // 2, W - mw // 3 + 1)), int(rng.integers(-mh // 2, H - mh // 3 + 1))


def _draw(kind, rng, st, cfg):
    g = st["g"]
    W, H = g["width"], g["height"]
    seed = int(rng.integers(0, 1 << 30))
    if kind == "resize":
        return _resize_to(rng, st)
    if kind in ("flatten", "bias_clear", "rig_clear", "init", "planes"):
        return [kind]
    if kind == "set_energy":                            # mostly across brightness / luma, either way: the planes a deep carver reads change
        now = 3 <= st["nrg"] <= 5
        return [kind, int(rng.choice([0, 1, 2, 6] if now else [3, 4, 5])) if rng.random() < 0.7 else int(rng.integers(0, 7))]
    if kind in ("bias_rgb", "rig_rgb"):
        mw, mh, xo, yo = _mask_args(rng, g)
        mch = int(rng.integers(1, 5))
        return [kind, seed, mw, mh, mch] + ([int(rng.choice([-40, -7, 0, 9, 60]))] if kind == "bias_rgb" else []) + [xo, yo]
    if kind in ("bias_f", "bias_dev", "rig_f", "rig_dev"):
        mw, mh, xo, yo = _mask_args(rng, g)
        if kind == "bias_f" and rng.random() < 0.3:     # lqr_carver_bias_add: a mask of the carver's size
            mw, mh, xo, yo = W, H, None, None
        op = [kind, seed, mw, mh] + ([int(rng.choice([-30, -5, 0, 7, 45]))] if kind.startswith("bias") else []) + [xo, yo]
        return op + ([str(rng.choice(["f4", "f8"]))] if kind.endswith("dev") else [])
    if kind in ("bias_xy", "rig_xy"):
        return [kind, seed, int(rng.integers(1, 300))]
    if kind in ("energy", "energy_dev"):
        form = int(rng.integers(0, 3))
        return [kind, form, int(rng.integers(0, 2)), int(rng.integers(0, 4)) if form == 2 else 2, int(rng.integers(0, 7)) if form == 2 else IT.GREY]
    if kind in ("read_sizes", "read_sizes_dev"):
        _, lo, hi = st["range"]
        return [kind, [int(s) for s in rng.integers(lo, hi + 1, int(rng.integers(1, 5)))]]
    if kind in ("forward_map", "forward_map_dev", "load_forward"):
        o = int(rng.integers(0, 2))
        if _room(H if o else W) < 1:                    # (the map's sizes go down to length - depth: no side below MIN_SIDE)
            o = 1 - o
        return [kind, _seams(rng, _room(H if o else W), 1), o]        # (a forward map's depth: any number of seams)
    if kind == "resize_forward":
        dw = int(rng.integers(-min(20, W - 5), min(12, W - 1)))
        dh = int(rng.integers(-min(12, H - 5), min(8, H - 1))) if rng.random() < 0.5 or dw == 0 else 0
        return [kind, W + dw, H + (dh if dw or dh else 1)]
    assert kind == "reopen"
    return [kind, str(rng.choice(["noinit", "device", "init", "init"]))]


# What leaves a plane stale if the host forgets to say so, and what would read the stale plane: an op of STALE in front of a
# CONSUMER with no flatten or transposition between them (a deeper resize the way the carver lies, a read-out in its own orientation).
# On a flat carver the planes are only there after a read-out: the PRIMER.
STALE = ("set_energy", "bias_clear", "rig_clear", "bias_rgb", "rig_rgb", "bias_f", "bias_dev", "rig_f", "rig_dev", "bias_xy", "rig_xy")


def _own_readout(rng, st):
    return [str(rng.choice(["energy", "energy_dev"])), int(rng.integers(0, 2)), st["g"]["orientation"], 2, IT.GREY]


def _consumer(rng, st):
    g, (_, lo, _) = st["g"], st["range"]
    if st["init"] and _room(lo) >= MIN_SEAMS and rng.random() < 0.6:
        s = lo - _seams(rng, _room(lo))
        return ["resize", g["width"], s] if g["orientation"] else ["resize", s, g["height"]]
    return _own_readout(rng, st)


WEIGHTS = {"resize": 6.0, "flatten": 1.0, "reopen": 0.6, "load_forward": 0.5, "resize_forward": 0.5, "init": 3.0}


def program(seed):
    """deterministic per seed; the oracle is run along to know the state every op is drawn in"""
    rng = np.random.default_rng([20261020, seed])
    kind, cls = TARGETS[seed % len(TARGETS)]
    need = OPS[kind]
    w = int(rng.integers(257, 331)) if rng.random() < 0.2 else int(rng.integers(24, 91))
    h = int(rng.integers(63, 131)) if rng.random() < 0.2 else int(rng.integers(8, 61))
    cfg = dict(nrg=int(rng.integers(0, 7)), delta=int(rng.choice([1, 2, 3])), rigidity=float(rng.choice([0.0, 0.0, 1.0, 8.0])),
               switch_freq=int(rng.choice([0, 1, 2, 3])), res_order=int(rng.integers(0, 2)), enl_step=float(rng.choice([1.2, 1.5, 2.0])),
               late_init=bool(rng.random() < 0.2), aux=bool(rng.random() < 0.3))
    plan = flag_plan(kind, cls, (seed // len(TARGETS)) % ROUNDS)
    # not initialised: a new carver (flat; transposed by a read-out), or one reopened without init
    via_reopen = not plan["init"] and cls not in _FLAT
    cfg["late_init"] = not plan["init"] and not via_reopen
    cfg["aux"] = plan["aux"]
    if need.get("plain") or via_reopen:
        cfg.update(rigidity=0.0, switch_freq=0)
    prog = dict(seed=int(seed), image=dict(seed=int(seed), w=w, h=h, ch=int(rng.integers(1, 5))), config=cfg, ops=[])
    sh = Shadow(prog)
    ops = prog["ops"]
    total = int(rng.integers(4, 11))

    def emit(op):
        ops.append(json.loads(json.dumps(op)))
        return sh.apply(ops[-1])

    def tail_kind(st):
        kinds = [k for k in OPS if _allowed(k, st, cfg)]
        p = np.array([WEIGHTS.get(k, 1.0) for k in kinds])
        return kinds[int(rng.choice(len(kinds), p=p / p.sum()))]

    try:
        # 1. the masks the round's plan asks for, first (they flatten); each in a form the state allows, with an effect
        for flag, kinds in (("bias", ("bias_f", "bias_dev", "bias_xy", "bias_rgb")), ("rig", ("rig_f", "rig_dev", "rig_xy", "rig_rgb"))):
            st = sh.state()
            kinds = [k for k in kinds if _allowed(k, st, cfg)]
            for _ in range(3):                          # (a factor or values of 0: nothing happened; another is drawn)
                if not plan[flag] or sh.state()[flag] or not kinds:
                    break
                emit(_draw(kinds[int(rng.integers(0, len(kinds)))], rng, st, cfg))
        # 2. towards the target's class, then the target
        if cfg["late_init"] and cls == "transposed-flat":
            emit(["energy", int(rng.integers(0, 3)), 1, 2, IT.GREY])
        for _ in range(4):
            st = sh.state()
            if not st["init"]:
                break
            step = _towards(rng, st, cls)
            if step is None:
                break
            emit(step)
        st = sh.state()
        if via_reopen and st["cls"] == cls:
            emit(["reopen", "noinit"])
            st = sh.state()
        if st["cls"] == cls and _allowed(kind, st, cfg):
            if kind in STALE and st["g"]["depth"] == 0 and rng.random() < 0.5 and len(ops) < 8:
                emit(_own_readout(rng, st))
                st = sh.state()
            emit(_draw(kind, rng, st, cfg))
            if kind in STALE and rng.random() < 0.7 and len(ops) < 10:
                emit(_consumer(rng, sh.state()))
        # 3. whatever the state allows
        while len(ops) < total:
            st = sh.state()
            if rng.random() < 0.07 and len(ops) >= 3 and len(ops) == total - 1 and st["mode"] == "oracle":
                emit(["bad_init"] if st["init"] and rng.random() < 0.5 else ["bad_resize", 0, st["g"]["height"]])
                break
            k = tail_kind(st)
            emit(_draw(k, rng, st, cfg))
            if k in STALE and st["mode"] == "oracle" and len(ops) < total and rng.random() < 0.4:
                emit(_consumer(rng, sh.state()))
    finally:
        sh.close()
    return prog
