"""Write tests/golden/workspace_sizes.json: what every workspace size query of libisd_hip.so answers (and what
isd_eegnet_sync_block / isd_paperhead_sync_block hand out) on a small grid of shapes around the places where rounding
can go wrong, refused arguments and their negative codes included.  An allocation size is behaviour that callers see:
tests/test_workspace_cpu.py and tests/test_workspace_gpu.py ask the same questions of the current build and compare.

The "cpu" section needs the library and no device; the "gpu" section (--gpu) needs a device for its plans and launches
nothing.  Run it from the commit whose answers the tests pin; a run without --gpu keeps the file's "gpu" section:
    python tools/make_workspace_golden.py [--gpu] [OUT.json]
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
PAC_BLOCK = 8                                                    # kPacBlock (csrc/pac.hip): T is padded to whole blocks
ENV_MAX_CHANNELS = 128
HEAD_C, HEAD_T, HEAD_BATCHES = 64, 800, (0, 1, 2, 350)           # tools/bench_*.py: trials of [64, 800], batches to 350
TS_SHAPE = (125, 62, 31, 15, 15, 32, 5)                          # taps at 250 Hz, num_T, num_S, hidden, classes


def _key(name, *args):
    return "%s(%s)" % (name, ", ".join(str(a) for a in args))


def _query(h, out, name, *args):
    out[_key(name, *args)] = int(getattr(h, name)(*args))


def _shortest_T(create):
    """The shortest trial a head's plan creator accepts, and its plan."""
    for T in range(1, 4096):
        plan = ctypes.c_void_p()
        if create(plan, T) == 0:
            return T, plan
    raise RuntimeError("no T below 4096 was accepted")


def _head_plans(h):
    """(label, plan, workspace query, destroy, sync entry point or None, its stage count) for the four heads."""
    makers = {
        "eegnet": (lambda p, T: h.isd_eegnet_plan_create(ctypes.byref(p), HEAD_C, 32, 64, T),
                   h.isd_eegnet_workspace_bytes, h.isd_eegnet_plan_destroy, h.isd_eegnet_sync_block, 3),
        "cvblock": (lambda p, T: h.isd_cvblock_plan_create(ctypes.byref(p), HEAD_C, 32, T),
                    h.isd_eegnet_workspace_bytes, h.isd_eegnet_plan_destroy, h.isd_eegnet_sync_block, 3),
        "paperhead": (lambda p, T: h.isd_paperhead_plan_create(ctypes.byref(p), HEAD_C, 32, T),
                      h.isd_paperhead_workspace_bytes, h.isd_paperhead_plan_destroy, h.isd_paperhead_sync_block, 4),
        "tsception": (lambda p, T: h.isd_tsception_plan_create(ctypes.byref(p), HEAD_C, T, *TS_SHAPE),
                      h.isd_tsception_workspace_bytes, h.isd_tsception_plan_destroy, None, 0),
    }
    for name, (create, query, destroy, sync, stages) in makers.items():
        T_min, plan = _shortest_T(create)
        yield "%s[T=%d]" % (name, T_min), plan, query, destroy, sync, stages
        plan = ctypes.c_void_p()
        assert create(plan, HEAD_T) == 0, h.isd_last_error()
        yield "%s[T=%d]" % (name, HEAD_T), plan, query, destroy, sync, stages


def cpu_cases(h):
    """{question: answer} for every query that needs no device."""
    out = {}
    for M, (K, N) in itertools.product((0, 1, 63, 64, 65, 16385), ((1, 1), (16, 5), (256, 32))):
        _query(h, out, "isd_linear_workspace_bytes", M, K, N)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0)):
        _query(h, out, "isd_linear_workspace_bytes", *bad)
    for B in (0, 1, 256, 257, -1):
        _query(h, out, "isd_softmax_ce_workspace_bytes", B)
    pac_T = (1, 4096, 100 * PAC_BLOCK - 1, 100 * PAC_BLOCK + 1)
    for rows, P, A, T, f64 in itertools.product((0, 1, 3), (1, 2), (1, 3), pac_T, (0, 1)):
        _query(h, out, "isd_pac_work_bytes", rows, P, A, T, f64)
    for bad in ((-1, 1, 1, 8), (1, 0, 1, 8), (1, 1, 0, 8), (1, 1, 1, 0), (1, 1, 1, 4097), (1 << 20, 1 << 10, 2, 8)):
        _query(h, out, "isd_pac_work_bytes", *bad, 0)
    for n, C, T, f64 in itertools.product((0, 1, 2), (1, 16, 17, ENV_MAX_CHANNELS), (0, 1, 795), (0, 1)):
        _query(h, out, "isd_envcorr_work_bytes", n, C, T, f64)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, ENV_MAX_CHANNELS + 1, 1), (1, 1, -1)):
        _query(h, out, "isd_envcorr_work_bytes", *bad, 0)
    for n, C, T, m, f64 in itertools.product((0, 1, 350), (1, 64, 65, 128), (1, 795), (1, 16, 64), (0, 1)):
        _query(h, out, "isd_ica_step_work_bytes", n, C, T, m, f64)
    for bad in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 129, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 65)):
        _query(h, out, "isd_ica_step_work_bytes", *bad, 0)
    for B, D, L in itertools.product((0, 1, 64, 65, -1), (16, 32), (1, 2)):
        _query(h, out, "isd_tail_fused_save_floats", B, 8, D, L)
        _query(h, out, "isd_tail_fused_workspace_floats", B, 7, 8, D, L, 5)
    for label, plan, query, destroy, sync, stages in _head_plans(h):
        for B in HEAD_BATCHES + (-1, 351):
            out[_key(query.__name__, label, B)] = int(query(plan, B))
        for B, backward, stage in itertools.product(HEAD_BATCHES, (0, 1), range(stages)):
            off, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
            rc = int(sync(plan, B, backward, stage, ctypes.byref(off), ctypes.byref(n)))
            out[_key(sync.__name__, label, B, backward, stage)] = [rc, off.value, n.value]
        destroy(plan)
        out[_key(query.__name__, "null", 1)] = int(query(None, 1))
    return out


def gpu_cases(h):
    """{question: answer} for the queries whose plan lives on the device; no kernel is launched."""
    import numpy as np
    import isd_amd
    from isd_amd import _lib
    out = {}
    window = _lib.double_array(np.hanning(257)[:256])
    psd = ctypes.c_void_p()
    _lib.check(h.isd_psd_plan_create(ctypes.byref(psd), 256, 256, 128, 0, 128, window, 256.0, 1))
    for rows, T, f64 in itertools.product((1, 64, 65), (2048, 256), (0, 1)):     # 15 segments are split over z, one is not
        _query_plan(h, out, "isd_psd_work_bytes", psd, rows, T, f64)
    for n, f64, over in itertools.product((0, 4), (0, 1), (0, 1)):
        _query_plan(h, out, "isd_csd_work_bytes", psd, n, 8, 1024, over, f64)
    before = h.isd_csd_chunk_bytes(60000)                        # room for one trial's spectra: three trials, three chunks
    try:
        for f64, over in itertools.product((0, 1), (0, 1)):
            out[_key("isd_csd_work_bytes[chunk=60000]", 3, 8, 1024, over, f64)] = int(
                h.isd_csd_work_bytes(psd, 3, 8, 1024, over, f64))
    finally:
        h.isd_csd_chunk_bytes(before)
    h.isd_psd_plan_destroy(psd)

    zones = isd_amd.zone_index_lists()
    routes = {"layerwise": (72, [list(range(72))], 17, 1, 17, 0),       # (c_total, zones, window, step, T, bf16)
              "fused_f32": (64, zones, 250, 125, 800, 0),
              "fused_bf16": (64, zones, 250, 125, 800, 1)}
    for label, (c_total, zs, W, step, T, bf16) in routes.items():
        plan = ctypes.c_void_p()
        _lib.check(h.isd_conv4_plan_create(ctypes.byref(plan), c_total, len(zs), _lib.int_array([len(z) for z in zs]),
                                           _lib.int_array([i for z in zs for i in z]), 32, 4, W, step))
        _lib.check(h.isd_conv4_plan_set_activation_dtype(plan, bf16))
        for B in (0, 1, 2, 64):
            out[_key("isd_conv4_workspace_bytes", label, B, T)] = int(h.isd_conv4_workspace_bytes(plan, B, T))
        h.isd_conv4_plan_destroy(plan)

    fx = isd_amd.FeatureExtractor(512, 256.0, isd_amd.BANDS_9)
    for B, C in ((1, 1), (1, 64), (1, 65), (5, 13)):
        out[_key("isd_features_backward_workspace_bytes", B, C)] = int(
            h.isd_features_backward_workspace_bytes(fx.fb._h, fx.stft._h, B, C, fx._klo, fx._khi))
    return out


def _query_plan(h, out, name, plan, *args):
    out[_key(name, *args)] = int(getattr(h, name)(plan, *args))


def main():
    from isd_amd import _lib
    args = [a for a in sys.argv[1:] if a != "--gpu"]
    path = args[0] if args else GOLDEN
    golden = json.load(open(path)) if os.path.exists(path) else {}
    golden["cpu"] = cpu_cases(_lib.lib())
    if "--gpu" in sys.argv:
        golden["gpu"] = gpu_cases(_lib.lib())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, {k: len(v) for k, v in golden.items()})


if __name__ == "__main__":
    main()
