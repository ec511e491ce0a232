"""Cost of a frame rendered on the device against the read-back it replaces.

At each bench configuration (default c1 and c2), on one handle after 2 steps,
with a 1920 x 1080 image of the whole domain, medians of 5 fenced host calls
(cfd_synchronize on both sides; the first call of each kind is a warm-up and
is not counted):
  map           set_view(1920, 1080): the ownership map, once per view
  speed_fixed   render("speed", range=(0, 1.5)): the shade pass and the copy of
                4 W H bytes to the host
  speed_auto    render("speed"): the same after the range reduction
  vorticity     render("vorticity"): the same after the derived pass (k_flow_diag
                with its field outputs) and the range reduction
  readback      get_u() + get_p(): the parent commit's path to a frame (N cells
                to the host, widened to 24 N bytes of doubles), before any drawing
shade_device_us is the shade kernel alone: (render with a fixed range) - (the
copy of the image alone, timed as render_owner(), the same number of bytes
from the same kind of buffer); its bytes are 8 W H (the map read, the pixel
written) plus the gathered values counted once per covered cell: 8 B per cell
of u, over the cells that own a pixel.
Writes profiles/r13/render_cost.json.

    python tools/render_cost.py [--configs c1 c2] [--mesh-cache-dir DIR] [--png FILE]

--png: also write a C0 (Voronoi) speed frame there through cfd2_amd.image.write_png.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo2_amd"))
sys.path.insert(0, ROOT)

H = {"c1": 0.001723, "c2": 5.449e-4}  # bench.py CONFIGS
W_PX, H_PX = 1920, 1080


def fenced(s, fn, reps=5):
    ts = []
    for _ in range(reps + 1):  # the first call is the warm-up
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:]), min(ts[1:])


def solver_for(mesh):
    from cfd2_amd import GpuSolver, default_config
    s = GpuSolver(mesh, config=default_config(fixed_outer=5, fixed_inner=30))
    s.set_dt(1e-3)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(1)
    s.initialize_history()
    s.step()
    s.step()
    return s


def row_for(s, mesh, name, np):
    t0 = time.perf_counter()
    s.set_render_mesh(mesh)
    upload = time.perf_counter() - t0
    covered = s.set_view(W_PX, H_PX)
    m_med, m_min = fenced(s, lambda: s.set_view(W_PX, H_PX))
    owner = s.render_owner()
    cells_seen = int(len(np.unique(owner[owner != 0xFFFFFFFF])))
    f_med, f_min = fenced(s, lambda: s.render("speed", range=(0.0, 1.5)))
    a_med, a_min = fenced(s, lambda: s.render("speed"))
    v_med, v_min = fenced(s, lambda: s.render("vorticity"))
    c_med, c_min = fenced(s, s.render_owner)
    r_med, r_min = fenced(s, lambda: (s.get_u(), s.get_p()))
    shade = f_med - c_med
    shade_bytes = 8.0 * W_PX * H_PX + 8.0 * cells_seen
    return dict(config=name, cells=mesh.num_cells(), width=W_PX, height=H_PX, covered_pixels=covered,
                cells_on_image=cells_seen, polygon_upload_ms=1e3 * upload,
                map_ms=1e3 * m_med, map_min_ms=1e3 * m_min,
                speed_fixed_ms=1e3 * f_med, speed_fixed_min_ms=1e3 * f_min,
                speed_auto_ms=1e3 * a_med, speed_auto_min_ms=1e3 * a_min,
                vorticity_ms=1e3 * v_med, vorticity_min_ms=1e3 * v_min,
                image_copy_ms=1e3 * c_med, image_copy_min_ms=1e3 * c_min,
                readback_ms=1e3 * r_med, readback_min_ms=1e3 * r_min,
                shade_device_us=1e6 * shade, shade_bytes=shade_bytes,
                shade_gbs=shade_bytes / shade / 1e9 if shade > 0 else None,
                frame_over_readback=a_med / r_med, faster="frame" if a_med < r_med else "readback",
                render_range=[float(v) for v in s.last_render_range])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(H))
    ap.add_argument("--mesh-cache-dir", default=None, help="load / save <dir>/<config>.mesh (bench.py --mesh-cache files)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "render_cost.json"))
    ap.add_argument("--png", default=None, help="write a C0 speed frame (960 x 320) to this file")
    args = ap.parse_args()
    import numpy as np
    from cfd2_amd import build_id, image
    from cfd2_amd.mesh import Mesh, bench_channel, bench_voronoi_channel

    if args.png:
        mesh = bench_voronoi_channel()
        s = solver_for(mesh)
        s.set_render_mesh(mesh)
        covered = s.set_view(960, 320)
        img = s.render("speed")
        image.write_png(args.png, img)
        print(json.dumps(dict(png=args.png, cells=mesh.num_cells(), covered=covered,
                              range=[float(v) for v in s.last_render_range],
                              opaque=int((img[:, :, 3] == 255).sum()))), flush=True)
        s.close()
        del mesh
    rows = []
    for name in args.configs:
        cache = os.path.join(args.mesh_cache_dir, name + ".mesh") if args.mesh_cache_dir else None
        if cache and os.path.exists(cache):
            mesh = Mesh.load(cache)
        else:
            mesh = bench_channel(H[name], 100)
            if cache:
                mesh.save(cache)
        s = solver_for(mesh)
        row = row_for(s, mesh, name, np)
        row["build"] = build_id()
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="one handle after 2 steps (fixed schedule 5 Picard x 30 FGMRES / AMG, dt 1e-3), a 1920 x 1080 "
                            "image of the whole domain (tools/render_cost.py): medians of 5 fenced host calls each. map = "
                            "set_view; speed_fixed / speed_auto / vorticity = render() with a fixed range, with the auto "
                            "range, and of the derived field; image_copy = render_owner(), the copy of 4 W H bytes alone; "
                            "readback = get_u() + get_p(); shade_device_us = speed_fixed - image_copy over 8 W H bytes plus "
                            "8 B per cell that owns a pixel",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
