"""CPU tier of the primitive tests: the numpy models of pmg_wave.h (tests/wave_models.py) against the emulator's stand-in
header tests/emu/pmg_wave.h, through the SAME probe bodies the device probe library runs on the shipped header
(gpu_probe/pmg_prim_probe.inc, tests/test_gpu_wave_primitives.py) -- models and stand-in check each other before any
GPU time is spent, and the two headers are held to one specification.  Plus the build-time checks of the device probe
libraries themselves: exported symbols, and no DPP hazard around the inline-asm blocks in THEIR code either."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import wave_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, 'gpu_probe')
PROBE_LIBS = ['libpmg_gpu_probe.so', 'libpmg_gpu_probe_plain.so']
PROBE_SYMBOLS = ['pmgd_variant', 'pmgd_prim', 'pmgd_prim_nin', 'pmgd_prim_nout', 'pmgd_prim_families', 'pmgd_dynamics', 'pmgd_ik',
                 'pmgd_narrowphase', 'pmgd_fk64', 'pmgd_cyl_redo64', 'pmgd_cyl_redo64_pairs', 'pmgd_double_maths']


@pytest.fixture(scope='module')
def emu_prim(emu_library):
    lib = C.CDLL(emu_library.path)
    assert (lib.pmge_prim_nin(), lib.pmge_prim_nout(), lib.pmge_prim_families()) == (M.NIN, M.NOUT, len(M.FAMILIES))
    return lib.pmge_prim


@pytest.mark.parametrize('ns,fam,ctx', M.cases())
def test_emulator_primitive_matches_model(emu_prim, ns, fam, ctx):
    # wr::any_row_mask: the device ORs the four rows of the wavefront; the stand-in documents that its rows may have
    # diverged and lets each row answer for itself -- the one primitive the two headers define differently
    M.check_against_model(emu_prim, ns, fam, ctx, any_row_mask_per_row=True)


def test_models_tell_a_wrong_source_lane_apart():
    """the inputs are distinct in every lane and slot: a model evaluated with a neighbouring lane argument differs"""
    inp = M.exact_inputs(1)
    full = np.ones(64, bool)
    for ns in ('wv', 'wr'):
        a, da = M.model(ns, 'bcast', inp, full, 3)
        b, _ = M.model(ns, 'bcast', inp, full, 4)
        assert M.mismatches(a, b, da)
    assert len(set(inp.ravel().tolist())) == inp.size


def _hazard_tool():
    spec = importlib.util.spec_from_file_location('check_dpp_hazards', os.path.join(ROOT, 'tools', 'check_dpp_hazards.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', PROBE_LIBS)
def test_probe_library_exports_every_probe_and_has_no_dpp_hazard(built, name):
    """tools/check_dpp_hazards.py proves for libpmg_hip.so that no VALU write of EXEC sits inside the 5 wait states of a DPP
    instruction and no VALU write of its source inside 2; the inline-asm blocks of pmg_wave.h rely on it.  The same on the
    probe libraries: a probe that misbehaves on the GPU is then the primitive, not the probe's surroundings."""
    path = os.path.join(PROBE_DIR, name)
    assert os.path.exists(path), 'build() did not produce %s' % name
    lib = C.CDLL(path)
    for sym in PROBE_SYMBOLS:
        assert hasattr(lib, sym), '%s does not export %s' % (name, sym)
    assert lib.pmgd_variant() == PROBE_LIBS.index(name)
    assert (lib.pmgd_prim_nin(), lib.pmgd_prim_nout(), lib.pmgd_prim_families()) == (M.NIN, M.NOUT, len(M.FAMILIES))
    tool = _hazard_tool()
    ndpp, bad_exec, bad_src, _ = tool.check_binary(tool.disassemble(path))
    assert ndpp > 100, ndpp
    assert bad_exec == 0 and bad_src == 0, (bad_exec, bad_src)
