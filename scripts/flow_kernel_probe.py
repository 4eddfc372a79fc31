"""The flow-image kernels next to the time-image kernels, for a kernel trace: on a 1M-event slice of
the given sensor, after a short solve, `reps` colour-coded time images at scale 3 (k_color_point, k_color_final) and `reps`
colour-coded flow images (k_flow_owner, k_flow_field), both ownership rules alternating.  Run under a kernel tracer:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/flow_kernel_probe.py 346 260
usage: flow_kernel_probe.py <columns> <rows> [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from better_flow_amd import accel, synth  # noqa: E402

W, H = int(sys.argv[1]), int(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
sl = synth.make_slice(1000000, H, W, 0.03, seed=1)
a = accel.Accel(max_events=len(sl["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
a.set_cloud(3, H, W)
o = a.default_opts()
o.res_x, o.res_y, o.max_iter = H, W, 40
a.run(o)
for k in range(reps):
    a.color_time_img(3, H, W, show_final=False)
    a.color_flow_img(H, W, k & 1)
owner, _, _ = a.flow_field(H, W)
print("%d x %d: %d events, %d pixels covered (%.1f events per covered pixel)" % (W, H, len(sl["t"]), (owner >= 0).sum(), len(sl["t"]) / max(1, (owner >= 0).sum())))
a.close()
