"""CPU: the library's options (mal_set_option / mal_get_option) -- the accepted names, their documentation, their ranges, and
the automatic task decomposition under "device_cus" (no kernel is launched, no device is queried)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARCH = os.path.join(ROOT, "mal_amd", "csrc", "mal_march.hip")


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _body(name):
    src = open(MARCH).read()
    start = src.index('extern "C" int %s(' % name)
    return src[start:src.index("\n}\n", start)]


def set_names():
    return re.findall(r'eq\("([a-z0-9_]+)"\)', _body("mal_set_option"))


def get_names():
    return re.findall(r'\{"([a-z0-9_]+)", &g_', _body("mal_get_option"))


def header_names():
    text = open(os.path.join(ROOT, "include", "mal_hip.h")).read()
    block = text[text.index("/* ---- library options"):text.index("int mal_set_option(")]
    return re.findall(r'"([a-z0-9_]+)"', block)


def _get(lib, name):
    v = ctypes.c_int(-12345)
    assert lib.mal_get_option(name.encode(), ctypes.byref(v)) == 0, name
    return v.value


def test_every_option_is_swept_or_excluded_with_a_reason():
    from tests.test_gpu_schedule import EXCLUDED, SWEPT
    names = set_names()
    assert len(names) == len(set(names)) >= 20
    assert not set(SWEPT) & set(EXCLUDED)
    assert set(names) == set(SWEPT) | set(EXCLUDED), (sorted(set(names) - set(SWEPT) - set(EXCLUDED)),
                                                      sorted(set(SWEPT) | set(EXCLUDED) - set(names)))
    assert all(len(r) > 20 for r in EXCLUDED.values())


def test_header_documents_exactly_the_accepted_names():
    assert sorted(set(header_names())) == sorted(set_names())
    assert sorted(get_names()) == sorted(set_names())


def test_get_option_round_trip(lib):
    for name in set_names():
        v = _get(lib, name)
        assert lib.mal_set_option(name.encode(), v) == 0, (name, v)
        assert _get(lib, name) == v
    assert lib.mal_get_option(b"fwd_waves", ctypes.byref(ctypes.c_int())) == -1
    assert lib.mal_get_option(b"march_rows", None) == -1
    assert lib.mal_set_option(b"fwd_waves", 1) == -1
    old = _get(lib, "syn_rows")
    try:
        assert lib.mal_set_option(b"syn_rows", 7) == 0 and _get(lib, "syn_rows") == 7
    finally:
        lib.mal_set_option(b"syn_rows", old)


def test_experiments_only_switches_are_refused_in_the_default_build(lib):
    if lib.mal_build_has_experiments():
        pytest.skip("library built with -DMAL_EXPERIMENTS")
    for name in ("temporal_spec", "march3", "syn_queue"):
        assert lib.mal_set_option(name.encode(), 1) == -1, name
        assert lib.mal_set_option(name.encode(), 0) == 0, name
    assert lib.mal_set_option(b"pass_impl", 0) == -1 and lib.mal_set_option(b"pass_impl", 2) == -1


def test_decomposition_option_ranges(lib):
    saved = {n: _get(lib, n) for n in ("pack_rows", "march_rows", "march_rows_fwd", "device_cus", "syn_rows")}
    try:
        # the packing sweep's smoothness partials (8 doubles per task) are sized for 8-row tasks (ws_blocks): fewer rows would
        # write past StepWs.bs_p / DrWs.sm[0]
        for v in (0, 4, 7, 4097):
            assert lib.mal_set_option(b"pack_rows", v) == -1, v
        for v in (8, 9, 4096):
            assert lib.mal_set_option(b"pack_rows", v) == 0 and _get(lib, "pack_rows") == v
        for name in ("march_rows", "march_rows_fwd"):
            assert lib.mal_set_option(name.encode(), -1) == -1 and lib.mal_set_option(name.encode(), 4097) == -1
        assert lib.mal_set_option(b"device_cus", -1) == -1 and lib.mal_set_option(b"device_cus", 65537) == -1
        assert lib.mal_set_option(b"syn_rows", 1) == -1 and lib.mal_set_option(b"syn_rows", 65) == -1
    finally:
        for n, v in saved.items():
            lib.mal_set_option(n.encode(), v)


def _geometry(lib, B, H, W, flags):
    s, g, r, it = (ctypes.c_int() for _ in range(4))
    assert lib.mal_march_geometry(B, H, W, flags, ctypes.byref(s), ctypes.byref(g), ctypes.byref(r), ctypes.byref(it)) == 0
    return s.value, g.value, r.value


def test_device_cus_pins_the_automatic_decomposition(lib):
    """at B=12 192x640 (the gradient passes: 60-column strips, CUs x 8 wave slots): 256 CUs (MI355X) give 13 rows, 1980 tasks
    in one round; 32 CUs (one CPX partition) give one segment per strip; 304 (MI300X) 11 rows"""
    saved = {n: _get(lib, n) for n in ("device_cus", "march_rows", "march_rows_fwd")}
    try:
        lib.mal_set_option(b"march_rows", 0)
        lib.mal_set_option(b"march_rows_fwd", 0)
        grad = 2  # MAL_F_GRAD
        for cus, want in ((256, (11, 15, 13)), (32, (11, 1, 192)), (304, (11, 18, 11)), (1024, (11, 24, 8))):
            assert lib.mal_set_option(b"device_cus", cus) == 0
            assert _geometry(lib, 12, 192, 640, grad) == want, cus
            s, g, r = _geometry(lib, 12, 192, 640, grad)
            assert 12 * s * g <= cus * 8 or r == 8
        # the explicit row count wins over the device size; fewer than 8 rows act as 8 (the workspace's minimum)
        lib.mal_set_option(b"march_rows", 9)
        assert _geometry(lib, 12, 192, 640, grad)[2] == 9
        lib.mal_set_option(b"march_rows", 3)
        assert _geometry(lib, 12, 192, 640, grad)[2] == 8
    finally:
        for n, v in saved.items():
            lib.mal_set_option(n.encode(), v)


def test_stale_decomposition_has_its_own_error(lib):
    assert b"decomposition" in lib.mal_strerror(-6)
