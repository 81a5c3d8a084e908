"""The carver-control calls of include/lqr_control.h as data: the sequences recorded from the genuine liblqr under tests/golden/control/
(scripts/ref_engine/make_control_golden.py), the driver that runs one on any carver class (the genuine code's, the engine's binding),
and the engine's rules as a model of the return values and progress events, which tests/test_control_golden.py holds against what
the genuine code gave.

A spec: w, h, seed (the image, datasets.photo_like), aux (attached carvers), kw (Carver.configure), ops.  Ops:
    ["cancel"] / ["cancel_aux", i]        lqr_carver_cancel on the carver / on its i-th attached carver, outside any call
    ["arm", n, target]                    the next resize cancels `target` (-1 the carver, i its i-th attached one) from its n-th update callback
    ["resize", w1, h1] ["flatten"] ["dump"] ["scan"]
    ["dump_vmaps"] ["no_dump_vmaps"] ["use_cache", on] ["gradient", gf] ["energy"]
    ["foreach", recursive, stop_at, stop_ret]
"""
import json

import numpy as np

import datasets as D

LQR_ERROR, LQR_OK, LQR_NOMEM, LQR_USRCANCEL = 0, 1, 2, 3
W, H = 64, 48
# LqrGradFuncType -> LqrEnergyFuncBuiltinType, as liblqr 0.4.1's lqr_carver_set_gradient_function maps them (NORM_BIAS and YABS have no
# builtin energy left and become the null energy)
GRADIENT_TO_BUILTIN = {0: 0, 1: 6, 2: 1, 3: 2, 4: 6, 5: 6}

RULES_NOTE = ("the engine's rules (include/lqr_control.h): a cancel outside a call changes nothing and returns LQR_OK; a cancel from the "
              "n-th update callback ends the resize with LQR_USRCANCEL after exactly n update events and without an end event; every later "
              "resize and flatten returns LQR_USRCANCEL, lqr_vmap_dump and the scans still serve; lqr_carver_cancel on an attached carver "
              "returns LQR_ERROR and touches nothing.  Where the engine departs (finding half_built_state): after a cancelled resize the "
              "genuine carver is left inside the session it was building (width, depth and map are those of a half-built map); the engine "
              "holds the state after the last completed session.")


def _spec(ops, aux=0, seed=3, **kw):
    return dict(w=W, h=H, seed=seed, aux=aux, kw=kw, ops=ops)


def cases():
    out = [
        ("idle_cancel_then_resize", _spec([["cancel"], ["resize", 50, 48], ["cancel"], ["resize", 50, 40]])),
        ("set_no_dump_vmaps", _spec([["dump_vmaps"], ["resize", 58, 48], ["no_dump_vmaps"], ["resize", 52, 48], ["dump_vmaps"], ["resize", 52, 44]])),
        ("use_cache_off", _spec([["use_cache", 0], ["resize", 50, 40], ["dump"]])),
        ("use_cache_off_then_on", _spec([["use_cache", 0], ["resize", 56, 48], ["use_cache", 1], ["resize", 50, 44]])),
        ("foreach", _spec([["foreach", 0, 0, 0], ["foreach", 1, 0, 0], ["foreach", 0, 2, 0], ["foreach", 1, 2, 2], ["foreach", 0, 2, 3]], aux=3)),
        ("foreach_empty", _spec([["foreach", 0, 0, 0], ["foreach", 1, 1, 0]])),
        ("cancel_aux_idle", _spec([["cancel_aux", 0], ["resize", 56, 48]], aux=1)),
    ]
    out.append(("cancel_aux_in_resize", _spec([["arm", 6, 0], ["resize", 50, 48], ["resize", 50, 40]], aux=1)))      # refused: the resize runs on
    for gf in range(6):
        out.append(("gradient_%d" % gf, _spec([["gradient", gf], ["energy"], ["resize", 54, 48]])))
    return out


def finding_cases():
    """sequences in which a cancel interrupts a session: the return values and events are the engine's, the carver's state afterwards is
    where it departs from liblqr (RULES_NOTE)"""
    after = [["resize", 44, 36], ["flatten"], ["dump"], ["scan"], ["cancel"], ["resize", 64, 48]]
    out = []
    for name, n in (("early", 2), ("middle", 10), ("last", 20)):                    # 64 -> 44: 20 reports
        out.append(("cancel_first_%s" % name, _spec([["arm", n, -1], ["resize", 44, 36]] + after)))
    for name, n in (("early", 22), ("middle", 26), ("last", 32)):                   # then 48 -> 36: 12 more
        out.append(("cancel_second_%s" % name, _spec([["arm", n, -1], ["resize", 44, 36]] + after)))
    out.append(("cancel_second_vert_first", _spec([["arm", 12 + 7, -1], ["resize", 44, 36]] + after, res_order=1)))
    out.append(("cancel_enlarge_second_step", _spec([["arm", 31 + 6, -1], ["resize", 110, 48]] + after, enl_step=1.5)))   # 64 -> 95 -> 110
    out.append(("cancel_enlarge_first_step", _spec([["arm", 9, -1], ["resize", 110, 48]] + after, enl_step=1.5)))
    out.append(("cancel_root_with_aux", _spec([["arm", 6, -1], ["resize", 50, 48]] + after, aux=1)))
    out.append(("cancel_with_dumps", _spec([["dump_vmaps"], ["arm", 24, -1], ["resize", 44, 36]] + after)))
    return out


def make_input(spec):
    img = D.photo_like(spec["w"], spec["h"], spec["seed"])
    aux = [D.noise(spec["w"], spec["h"], 900 + spec["seed"] + i)[:, :, :3].copy() for i in range(spec["aux"])]
    return img, aux


def run(api, carver_class, spec, img, aux_imgs):
    """the sequence on a fresh carver: a dict of arrays plus "record" (json: rets, getters and events after every op, the armed calls'
    results, lists)"""
    kw = dict(nrg_func=2, res_order=0, switch_freq=2, enl_step=2.0, dump_vmaps=False, progress=True)
    kw.update(spec["kw"])
    c = carver_class(api, img)
    c.configure(**kw)
    auxes = [c.attach(a) for a in aux_imgs]
    out, rets, getters, n_events, hooks, lists = {}, [], [], [], {}, {}
    armed = False
    for i, op in enumerate(spec["ops"]):
        k = op[0]
        ret = None
        if k == "cancel":
            ret = c.cancel()
        elif k == "cancel_aux":
            ret = auxes[op[1]].cancel()
        elif k == "arm":
            c.cancel_at_update(op[1], None if op[2] < 0 else auxes[op[2]])
            armed = True
        elif k == "resize":
            ret = c.resize(op[1], op[2])
            if armed:
                fired, hret = c.cancel_result()
                hooks[str(i)] = [int(fired), int(hret)]
                c.cancel_at_update(0)
                armed = False
            out["image@%d" % i] = c.read_image()
            for j, a in enumerate(auxes):
                out["aux%d_image@%d" % (j, i)] = a.read_image()
        elif k == "flatten":
            ret = c.flatten()
        elif k == "dump":
            try:
                m = c.vmap_dump()
                out["dump@%d" % i] = m["data"]
                lists["dump_meta@%d" % i] = [m["depth"], m["orientation"]]
                ret = 1
            except AssertionError:
                ret = 0
        elif k == "scan":
            ret = c.scan_rets()
        elif k == "dump_vmaps":
            c.set_dump_vmaps()
        elif k == "no_dump_vmaps":
            c.set_no_dump_vmaps()
        elif k == "use_cache":
            c.set_use_cache(op[1])
        elif k == "gradient":
            c.set_gradient_function(op[1])
        elif k == "energy":
            out["energy@%d" % i] = c.energy()
        elif k == "foreach":
            ret, visited, toks = c.list_foreach(recursive=bool(op[1]), stop_at=op[2], stop_ret=op[3], token=0x5a5a0000 + i)
            lists["foreach@%d" % i] = [visited, [int(t == 0x5a5a0000 + i) for t in toks]]
        else:
            raise ValueError(k)
        rets.append(ret)
        getters.append(c.getters())
        n_events.append(len(c.events))
    lists["dumped_depths"] = [int(v["depth"]) for v in c.dumped_vmaps()]
    rec = dict(rets=rets, getters=getters, n_events=n_events, events=[list(e) for e in c.events], hooks=hooks, lists=lists)
    out["record"] = np.array(json.dumps(rec, sort_keys=True))
    c.destroy()
    return out


# ---- the engine's rules as a model: return values and events ----------------------------------------------------------------------
def reports_of(spec, w_from, h_from, w1, h1):
    """the update events a complete resize fires per session: [(direction, seams)] in the order carved; every seam reports at these
    sizes (liblqr's update step 0.02: fewer than 50 seams per direction)"""
    kw = spec["kw"]
    enl = kw.get("enl_step", 2.0)
    dirs = [("w", w_from, w1), ("h", h_from, h1)]
    if kw.get("res_order", 0) == 1:
        dirs.reverse()
    out = []
    for d, a, b in dirs:
        if b == a:
            continue
        steps = []
        if b < a:
            steps.append(a - b)
        else:
            cur = a
            while cur < b:
                nxt = min(b, int(np.float32(cur) * np.float32(enl)) - 1)         # liblqr: one column short of enl_step times the width
                steps.append(nxt - cur)
                cur = nxt
        assert sum(steps) < 50
        out.append((d, steps))
    return out


def predict(spec):
    """what the engine's rules say each op returns and how many progress events the sequence has fired after it; None where the rules
    say nothing (no return value).  The sizes after a cancelled resize are the engine's (the last completed session)."""
    w, h = spec["w"], spec["h"]
    cancelled = False
    armed = None
    rets, n_events, sizes, hooks = [], [], [], {}
    ev = 0
    for i, op in enumerate(spec["ops"]):
        k, ret = op[0], None
        if k == "cancel":
            ret = LQR_OK
        elif k == "cancel_aux":
            ret = LQR_ERROR
        elif k == "arm":
            armed = (op[1], op[2])
        elif k == "resize":
            if cancelled:
                ret = LQR_USRCANCEL
            else:
                ret = LQR_OK
                seen = 0
                for d, steps in reports_of(spec, w, h, op[1], op[2]):
                    ev += 1                                     # init
                    for s in steps:
                        if armed and armed[1] < 0 and seen < armed[0] <= seen + s:
                            ev += armed[0] - seen
                            ret = LQR_USRCANCEL
                            cancelled = True
                            break
                        seen += s
                        ev += s
                        if d == "w":
                            w += s if op[1] > w else -s
                        else:
                            h += s if op[2] > h else -s
                    if ret != LQR_OK:
                        break
                    ev += 1                                     # end
                if armed:
                    fired = int(ret == LQR_USRCANCEL or (armed[1] >= 0 and armed[0] <= seen))
                    hooks[str(i)] = [fired, (LQR_OK if armed[1] < 0 else LQR_ERROR) if fired else 0]
            armed = None
        elif k == "flatten":
            ret = LQR_USRCANCEL if cancelled else LQR_OK
        elif k == "dump":
            ret = 1
        elif k == "scan":
            ret = [1, 1]
        elif k == "foreach":
            n = spec["aux"]
            ret = op[3] if 0 < op[2] <= n else LQR_OK
        rets.append(ret)
        n_events.append(ev)
        sizes.append((w, h))
    return dict(rets=rets, n_events=n_events, sizes=sizes, hooks=hooks)
