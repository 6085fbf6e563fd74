"""Where the HOST time of the autograd-API step goes: cProfile over N steps of render -> recon_data -> backward (the C++ autograd nodes),
top functions by own time.   python profiles/tools/api_cprofile.py [steps] [fused]"""
import sys, importlib, os, time, cProfile, pstats, io, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("3d-magic-mirror_amd")
dev = torch.device("cuda:0")
LEAVES = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
fused = len(sys.argv) > 2 and sys.argv[2] == "fused"
dr = pkg.DiffRender(os.path.join(ROOT, "tests/golden/templates/smpl_uv_642.npz"), 128, emit_imnormal=False)
sets = []
for r in range(8):
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, 48, 128, 128, seed=r)
    datt = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}
    for k in LEAVES: datt[k] = datt[k].clone().requires_grad_(True)
    sets.append((datt, gt.to(dev)))
def one(i):
    datt, gtd = sets[i % 8]
    for k in LEAVES: datt[k].grad = None
    if fused:
        loss, rgbs, _ = dr.render_recon(gtd, no_mask=True, **datt)
    else:
        rgbs, _ = dr.render(no_mask=True, **datt)
        loss = dr.recon_data(rgbs, gtd, no_mask=True)
    loss.backward()
for i in range(50): one(i)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(N): one(i)
t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
print("%s: host %.1f us/step, wall %.1f us/step" % ("render_recon" if fused else "render + recon_data", (t1 - t0) / N * 1e6, (t2 - t0) / N * 1e6))
pr = cProfile.Profile(); pr.enable()
for i in range(N): one(i)
pr.disable(); torch.cuda.synchronize()
s = io.StringIO(); pstats.Stats(pr, stream=s).sort_stats("tottime").print_stats(22); print(s.getvalue()[:6000])
