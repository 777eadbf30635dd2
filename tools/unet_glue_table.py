"""Per-U-Net-call kernel table of a rocprofv3 --kernel-trace database (rocpd SQLite) of
`bench.py --steps S`: every kernel's launches per call, average and ms per call, then the glue
kernels (torch elementwise / norm / copy, MIOpen transposes and tensor ops, and the p2p_unet.hip
kernels) split by launch grid, i.e. by shape.
Usage: python tools/unet_glue_table.py <run_results.db> <U-Net calls in the run>"""
import sqlite3
import sys

GLUE = ("CUDAFunctor_add", "direct_copy_kernel", "RowwiseMoments", "GroupNormKernelImpl", "ComputeFusedParams",
        "silu_kernel", "GeluCUDAKernelImpl", "BinaryFunctor", "batched_transpose", "SubTensorOp",
        "gn_stats_kernel", "gn_apply_nchw_kernel", "gn_apply_tok_kernel", "bias_residual_nchw_kernel",
        "bias_residual_tok_kernel", "geglu_kernel",
        # the transformer blocks' LayerNorms and the time path (torch's, then csrc/p2p_text.hip / p2p_unet.hip)
        "vectorized_layer_norm_kernel", "layer_norm_grouped_kernel", "layer_norm_kernel", "MT16x16x128",
        "time_linear_kernel")


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "")


def main(path, calls):
    c = sqlite3.connect(path)
    rows = c.execute("select name, duration, grid_x, grid_y, grid_z, workgroup_x from kernels").fetchall()
    tot = sum(r[1] for r in rows)
    print(f"{len(rows)} dispatches, {tot / 1e6:.2f} ms kernel time, {calls:g} U-Net calls -> "
          f"{tot / 1e6 / calls:.3f} ms per call (the warm-up group's convolution search included)")
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r[1])
    head = f"{'share%':>7} {'per call':>9} {'avg us':>9} {'ms/call':>8}  kernel"
    print("\n== every kernel\n" + head)
    for name, ds in sorted(by.items(), key=lambda kv: -sum(kv[1]))[:48]:
        print(f"{sum(ds) / tot * 100:7.2f} {len(ds) / calls:9.2f} {sum(ds) / len(ds) / 1e3:9.2f} "
              f"{sum(ds) / 1e6 / calls:8.3f}  {short(name)[:140]}")
    glue = {}
    for name, dur, gx, gy, gz, wx in rows:
        tag = next((g for g in GLUE if g in name), None)
        if tag:
            wgs = (gx // wx if wx else gx, gy, gz)
            glue.setdefault((tag, wgs, wx), []).append(dur)
    gtot = sum(sum(v) for v in glue.values())
    print(f"\n== glue kernels by launch grid: {gtot / 1e6 / calls:.3f} ms per call = {gtot / tot * 100:.2f}% of kernel time")
    print(f"{'per call':>9} {'avg us':>9} {'ms/call':>8}  kernel  workgroups x threads")
    for (tag, wgs, wx), ds in sorted(glue.items(), key=lambda kv: (kv[0][0], -sum(kv[1]))):
        if len(ds) / calls < 0.05:
            continue
        print(f"{len(ds) / calls:9.2f} {sum(ds) / len(ds) / 1e3:9.2f} {sum(ds) / 1e6 / calls:8.3f}  {tag}  {wgs} x {wx}")
    print("\n== glue kernels, totals\n" + f"{'per call':>9} {'avg us':>9} {'ms/call':>8}  kernel")
    tags = {}
    for (tag, _, _), ds in glue.items():
        tags.setdefault(tag, []).extend(ds)
    for tag, ds in sorted(tags.items(), key=lambda kv: -sum(kv[1])):
        print(f"{len(ds) / calls:9.2f} {sum(ds) / len(ds) / 1e3:9.2f} {sum(ds) / 1e6 / calls:8.3f}  {tag}")


if __name__ == "__main__":
    main(sys.argv[1], float(sys.argv[2]))
