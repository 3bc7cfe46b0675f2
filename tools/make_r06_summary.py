"""profiles/r06_summary.md: every kernel of the round-6 profile set against its byte model (from r06_traffic.json, the kernel-stats CSVs and the bench lines)."""
import csv, json, os
R = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles") + "/"
t = json.load(open(R + "r06_traffic.json"))


def stats(f):
    return {r["Name"].split("(")[0].replace("void ", ""): (int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in csv.DictReader(open(R + f))}


ks = stats("r06_bench_driver_cmd_kernel_stats.csv")
L = ["# Round 6: kernels against their byte models (MI355X, HBM peak 8.0 TB/s)\n",
     "Sources: `r06_bench_driver_cmd_kernel_stats.csv` (rocprofv3 --kernel-trace --stats over `python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --steady 0`: average launch),\n"
     "`r06_traffic.json` (separate `--pmc FETCH_SIZE` / `WRITE_SIZE` passes over the same command, `(2 x FETCH_SIZE + WRITE_SIZE) x 1024`), `r06_c*_kernel_stats.csv`, `r06_merge_kernel_stats.csv`.\n"
     "Kernel sources hash `%s` (`taichislam_amd.build.source_hash()`).  Made by `tools/make_r06_summary.py`.\n" % t["lib_source_hash"],
     "| kernel | launches | avg us | frames per launch | algorithmic MB per launch | counted HBM MB per launch | traffic / model | achieved GB/s (algorithmic) | of 8 TB/s |",
     "|---|---|---|---|---|---|---|---|---|"]


def row(name, kname, key):
    e = t.get(key)
    if not e or kname not in ks:
        return
    n, us = ks[kname]
    alg, hb, fpl = e.get("algorithmic_bytes_per_launch"), e["hbm_bytes_per_launch"], e.get("frames_per_launch")
    if alg:
        L.append(f"| `{name}` | {n} | {us:.1f} | {fpl:.2f} | {alg / 1e6:.1f} | {hb / 1e6:.1f} | {hb / alg:.2f}x | {alg / us / 1e3:.0f} | {alg / us / 1e3 / 8000:.3f} |")
    else:
        L.append(f"| `{name}` | {n} | {us:.1f} | {fpl:.2f} | - | {hb / 1e6:.1f} | - | - | - |")


row("k_integrate_batch (dominant)", [k for k in ks if "k_integrate_batch" in k][0], "integrate")
for short, key in (("k_voxelize_depth", "voxelize_depth"), ("k_segments", "segments"), ("k_scatter", "scatter"), ("k_plan", "plan"), ("k_apply_slab", "apply_slab")):
    kk = [k for k in ks if short in k]
    if kk:
        row(short, kk[0], key)
L += ["", "Other configurations (per unit of their bench line):\n",
      "| config | kernel(s) | unit | us per unit (HIP events / wall, bench line) | model MB | counted HBM MB | traffic / model | of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
for c, lab, unit, key in (("c1", "k_mc_summary + k_marching_cubes_lds", "mesh", "config1"), ("c3", "k_octo_depth_batch (8 queued frames per launch)", "frame", "config3"),
                          ("c4", "k_esdf_round x %.1f launches" % t["config4"]["launches_per_update"], "ESDF update", "config4"),
                          ("c4_wavefront", "k_esdf_wave x %.1f launches (esdf_mode 1)" % t["config4_wavefront"]["launches_per_update"], "ESDF update", "config4_wavefront")):
    j = json.load(open(R + f"r06_bench_{c}.json")); r = j["roofline"]; e = t[key]
    hb = e["hbm_bytes_per_launch"] / e.get("frames_per_launch", 1.0) if key == "config3" else e["hbm_bytes_per_launch"]
    alg, us = r["algorithmic_bytes_per_launch"], r["avg_launch_us"]
    L.append(f"| {c} ({j['value']:.0f} {j['unit']}) | `{lab}` | {unit} | {us:.1f} | {alg / 1e6:.2f} | {hb / 1e6:.2f} | {hb / alg:.2f}x | {alg / us / 1e3 / 8000:.4f} |")
ms = stats("r06_merge_kernel_stats.csv")
fk = [k for k in ms if "k_fuse_splat" in k]
if fk:
    n, us = ms[fk[0]]; hb = t["fuse_splat"]["hbm_bytes_per_launch"]
    L.append(f"| c5 on one GPU | `{fk[0].replace('tsl::', '')}` | splat of one 512^3 submap | {us:.0f} | ~84 (6 B per source voxel + 9 B per global voxel) | {hb / 1e6:.0f} | {hb / 84e6:.1f}x | {84e6 / us / 1e3 / 8000:.3f} |")
L += ["", "Round 5 for comparison (`r05_traffic.json`): Octomap 3.0 MB per frame (3.9x), `k_fuse_splat` 686 MB (8x) in 860 us, ESDF update 99.9 MB (4.1x), marching cubes 21.0 MB (3.9x), `k_integrate_batch` 1.43x.\n"]
open(R + "r06_summary.md", "w").write("\n".join(L) + "\n")
print("\n".join(L))
