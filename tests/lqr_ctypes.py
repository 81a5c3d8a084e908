"""Test-side binding: the package's ctypes mirror of the LqrCarver ABI
(gimp-lqr-plugin_amd/binding.py) plus the loaders of the two CHECKERS that only tests may use:
  * the CPU oracle      oracle/liblqr_oracle.so              (prefix "o")
  * a genuine liblqr-1  (prefix "", path from $LQR_REAL_LIB), where one exists.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as _ge

_pkg = _ge._import_package()
import importlib

_b = importlib.import_module("gimp_lqr_plugin_amd.binding")
from gimp_lqr_plugin_amd.binding import *          # noqa: F401,F403  (Api, Carver, engine_api, constants, helpers)
from gimp_lqr_plugin_amd.binding import _apis, _malloc_copy, _libc   # noqa: F401

ORACLE_LIB = os.path.join(ROOT, "oracle", "liblqr_oracle.so")

_engine_api = engine_api


def engine_api():
    """the package's engine_api(), plus the kernels' experiment switches from the environment (soaks and A/B runs of the tests and fuzz
    scripts): LQR_LV_DBG -> lqrhip_band_levels_debug (4 no near copy, 8 an image's slots on different XCDs, 16 timing jitter in an
    LQR_JITTER build), LQR_DPP_DBG -> lqrhip_dp_tile_debug (1 no near copies, 2 round 4's tile numbering, 4 timing jitter)"""
    import ctypes
    api = _engine_api()
    if not getattr(api, "_dbg_env_applied", False):
        api._dbg_env_applied = True
        for env, fn in (("LQR_LV_DBG", "lqrhip_band_levels_debug"), ("LQR_DPP_DBG", "lqrhip_dp_tile_debug")):
            if os.environ.get(env):
                f = getattr(api.lib, fn); f.argtypes = [ctypes.c_int]; f.restype = None
                f(int(os.environ[env]))
    return api


# What the oracle does not restate: it is 8-bit (no colour-depth surface), has no device, and leaves the normalised energy and the
# energy picture to tests/energy_cases.py (normalised / picture of its true plane).  bind_masks / bind_energy bind the rest.
ORACLE_ABSENT = frozenset(list(COLDEPTH_SYMBOLS) + [
    "lqrx_carver_bias_add_area_device", "lqrx_carver_rigmask_add_area_device", "lqrhip_debug_mask_flushes",
    "lqr_carver_get_energy", "lqr_carver_get_energy_image", "lqrx_carver_get_energy_device", "lqrx_carver_get_energy_image_device"])


def oracle_api():
    if "oracle" not in _apis:
        api = Api(ORACLE_LIB, "o")
        api.absent = ORACLE_ABSENT
        _apis["oracle"] = api
    return _apis["oracle"]


class OracleCarver(Carver):
    """binding.Carver on the oracle: the methods of the later surfaces that the case drivers (mask_cases.run, energy_cases.run,
    sequence_cases.run) call, in their 8-bit meaning"""

    depth = LQR_COLDEPTH_8I

    @classmethod
    def from_ext(cls, api, array, depth=None, init=True, delta_x=1, rigidity=0.0, preserve=False):
        assert depth in (None, LQR_COLDEPTH_8I) and not preserve, "the oracle is 8-bit"
        return cls(api, array, init=init, delta_x=delta_x, rigidity=rigidity)

    def attach_ext(self, array, depth=None):
        assert depth in (None, LQR_COLDEPTH_8I), "the oracle is 8-bit"
        aux = OracleCarver(self.api, array, init=False)
        ret = self.api.lqr_carver_attach(self.p, aux.p)
        assert ret == LQR_OK, ret
        self.aux.append(aux)
        return aux

    def scan_line_ext(self):
        img, count = self.read_scanlines()
        return img, list(range(count))

    def read_image_ext(self):
        return self.read_image()

    def energy_call(self, form, orientation, depth=LQR_COLDEPTH_32F, image_type=LQR_GREY_IMAGE, nbytes=0, guard=64, null=False):
        """lqr_carver_get_true_energy in C; the normalised form and the picture are energy_cases' models of that plane.  Arguments
        are refused as include/lqr_energy.h refuses them: nothing happens"""
        import numpy as np
        import energy_cases as EC
        a = bind_energy(self.api)
        buf = np.full(nbytes + guard, 0xa5, np.uint8)
        if null or orientation not in (0, 1) or (form == 2 and (depth not in COLDEPTH_DTYPES or image_type not in IMAGE_TYPE_CHANNELS)):
            return LQR_ERROR, buf
        h, w = self._image_size()
        true = np.zeros((h, w), np.float32)
        ret = a.lqr_carver_get_true_energy(self.p, true.ctypes.data, int(orientation))
        if ret != LQR_OK:
            return ret, buf
        res = true if form == 0 else EC.normalised(true) if form == 1 else EC.picture(true, depth, image_type)
        raw = np.ascontiguousarray(res).view(np.uint8).ravel()
        assert raw.size == nbytes, (raw.size, nbytes)
        buf[:nbytes] = raw
        return ret, buf


def real_liblqr_api():
    """A genuine liblqr-1, if $LQR_REAL_LIB points at one (second oracle)."""
    path = os.environ.get("LQR_REAL_LIB")
    if not path or not os.path.exists(path):
        return None
    api = Api(path, "", LIBLQR_SYMBOLS)
    api.has_ext = False
    return api
