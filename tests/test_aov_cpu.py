"""rt_aov_film (per-pixel second moment and first-hit planes) without a GPU: the struct layout against the header, argument
checks that never reach a device, the standard-error helper and the packed gather of the planes over gloo."""
import ctypes as C
import os
import shutil
import socket
import subprocess
import sys

import numpy as np

import rustraytracer_amd as rr
from rustraytracer_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "rt_abi.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_aov_film), offsetof(rt_aov_film, rgb_sq_sum),
           offsetof(rt_aov_film, albedo_sum), offsetof(rt_aov_film, normal_sum), offsetof(rt_aov_film, depth_sum),
           offsetof(rt_aov_film, n_hit), offsetof(rt_aov_film, n_aov), offsetof(rt_aov_film, aov_spp),
           offsetof(rt_aov_film, reserved), offsetof(rt_aov_film, aov_ms));
    return 0;
}
'''


def test_aov_film_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-x", "c", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    A = F.rt_aov_film
    want = [C.sizeof(A)] + [getattr(A, f).offset for f in ("rgb_sq_sum", "albedo_sum", "normal_sum", "depth_sum", "n_hit",
                                                           "n_aov", "aov_spp", "reserved", "aov_ms")]
    assert got == want
    assert C.sizeof(A) == 64
    # the existing structs keep their sizes: the planes add no field to rt_render_cfg or rt_stats
    assert C.sizeof(F.rt_render_cfg) == 80
    assert F.lib().rt_abi_version() == 5


def test_render_aov_rejects_null_handles_without_a_device():
    L = F.lib()
    cam = F.rt_camera()
    cfg = rr.make_cfg(8, 8, 1)
    aov = F.rt_aov_film()
    buf = np.zeros(8 * 8 * 3)
    aov.rgb_sq_sum = buf.ctypes.data
    fake = C.c_void_p(1)  # never dereferenced: the null argument is seen first
    for ctx, scene, camera in ((None, fake, C.byref(cam)), (fake, None, C.byref(cam)), (fake, fake, None)):
        assert L.rt_render_aov(ctx, scene, camera, C.byref(cfg), None, None, C.byref(aov), None) == F.RT_ERR_INVALID_ARG
        assert b"null" in L.rt_last_error()
        assert L.rt_render_aov_device(ctx, scene, camera, C.byref(cfg), None, None, C.byref(aov), None,
                                      None) == F.RT_ERR_INVALID_ARG
    assert L.rt_render_aov(fake, fake, C.byref(cam), None, None, None, None, None) == F.RT_ERR_INVALID_ARG


def test_standard_error_matches_numpy():
    rng = np.random.default_rng(7)
    H, W, S = 5, 7, 37
    samples = rng.gamma(0.7, 2.0, size=(S, H, W, 3)) * (rng.random((S, H, W, 1)) < 0.6)
    s = samples.sum(axis=0)
    sq = (samples * samples).sum(axis=0)
    n = np.full((H, W), S, dtype=np.uint32)
    se = rr.standard_error(s, sq, n)
    want = np.sqrt(np.var(samples, axis=0, ddof=1) / S)
    np.testing.assert_allclose(se, want, rtol=1e-9, atol=1e-12)
    # per-pixel counts differ (windows, progressive passes): each pixel uses its own n; n < 2 has no estimate
    n2 = np.arange(H * W, dtype=np.uint32).reshape(H, W) % 5
    s2 = np.zeros_like(s)
    sq2 = np.zeros_like(s)
    for k in range(S):
        m = (k < n2)[..., None]
        s2 += np.where(m, samples[k], 0.0)
        sq2 += np.where(m, samples[k] ** 2, 0.0)
    se2 = rr.standard_error(s2, sq2, n2)
    for y in range(H):
        for x in range(W):
            k = int(n2[y, x])
            if k < 2:
                assert np.isnan(se2[y, x]).all()
            else:
                np.testing.assert_allclose(se2[y, x], np.sqrt(np.var(samples[:k, y, x], axis=0, ddof=1) / k), rtol=1e-9,
                                           atol=1e-12)


WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["RR_ROOT"])
from rustraytracer_amd import dist as rd
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
W, H = 70, 41
window = (3, 5, 66, 38) if os.environ["RR_WINDOW"] == "1" else None
rng = np.random.default_rng(11)
full = [rng.standard_normal((H, W, 3)), rng.standard_normal((H, W)), rng.integers(0, 2**31, (H, W)).astype(np.int32)]
x0, y0, x1, y1 = window or (0, 0, W, H)
inside = np.zeros((H, W), dtype=bool)
inside[y0:y1, x0:x1] = True
for f in full:
    f[~inside] = 0
own = np.zeros(H * W, dtype=bool)
own[rd.owned_pixels(W, H, rank, world, window=window)] = True
own = own.reshape(H, W)
mine = [torch.from_numpy(np.where(own[..., None] if f.ndim == 3 else own, f, 0).astype(f.dtype)) for f in full]
g = rd.FilmGather(W, H, "cpu", window=window)
out = g.gather_planes(*mine)
assert all(a is b for a, b in zip(out, mine))
if rank == 0:
    for a, f in zip(mine, full):
        assert a.dtype == torch.from_numpy(f).dtype
        assert np.array_equal(a.numpy(), f), "gathered plane differs from the one-rank plane"
    print("OK", world, flush=True)
dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, window):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   RR_ROOT=ROOT, RR_WINDOW="1" if window else "0")
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert f"OK {world}" in outs[0]


def test_gather_planes_world2_gloo():
    _run(2, window=False)


def test_gather_planes_world3_gloo_window():
    _run(3, window=True)


def test_aov_kernels_are_in_the_library_and_use_no_scratch():
    """k_resolve_sq and k_aov are compiled for gfx950, once (binary64), and neither has a private segment: the traversal
    stack's overflow part of k_aov lives in a device buffer, its texture lookups are inlined."""
    blob = open(F.LIB_PATH, "rb").read()
    assert b"_ZN3rtd12k_resolve_sq" in blob and b"_ZN3rtd5k_aov" in blob
    assert b"_ZN5rtd325k_aov" not in blob
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources_so.py"), F.LIB_PATH],
                       stdout=subprocess.PIPE, text=True, check=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        cols = line.split()
        if cols and ("k_aov" in cols[0] or "k_resolve_sq" in cols[0]):
            rows[cols[0]] = cols
    assert len(rows) == 2, r.stdout
    for name, cols in rows.items():
        vgpr, agpr, spill, scratch = (int(x) for x in cols[1:5])
        assert spill == 0 and scratch == 0, (name, cols)
