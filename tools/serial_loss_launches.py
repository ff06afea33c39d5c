"""Config-5 training step of a source tree (argv[1], default: this repository): kernel launches per step, launches of the head
loss alone (forward + backward from leaf maps), host enqueue and step time (median of 5 windows of 20 steps), one JSON line.
A/B: KGDET_FUSED_SERIAL_LOSS=0, or the path of a checkout of another commit with its library built.
python tools/serial_loss_launches.py [tree]"""
import os, sys, time, json
ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
os.environ.setdefault('MIOPEN_USER_DB_PATH', os.path.join(ROOT, 'kgdet_amd', 'miopen_db', 'serial_train_fp32_b2'))
import torch
from torch.profiler import profile, ProfilerActivity
torch.backends.cudnn.benchmark = True
import kgdet_amd
assert os.path.abspath(kgdet_amd.__file__).startswith(ROOT), kgdet_amd.__file__
from kgdet_amd import build_detector, configs, synthetic
from kgdet_amd.dist import DistOptimizerHook
cfg = configs.reppoints_kp_r50_fpn()
torch.manual_seed(0)
model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=5e-3, momentum=0.9, weight_decay=1e-4, fused=True)
hook = DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2))
batch = synthetic.make_batch(2, 'cuda', seed=0)
def step():
    losses = model(batch['img'], batch['img_meta'], return_loss=True, gt_bboxes=batch['gt_bboxes'],
                   gt_labels=batch['gt_labels'], gt_keypoints=batch['gt_keypoints'])
    hook.step(model, opt, sum(sum(v) if isinstance(v, (list, tuple)) else v for v in losses.values()))
for _ in range(10): step()
torch.cuda.synchronize()
ts = []
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(20): step()
    t1 = time.time(); torch.cuda.synchronize(); t2 = time.time()
    ts.append(((t2 - t0) / 20 * 1e3, (t1 - t0) / 20 * 1e3))
ts.sort()
def kernels(prof):
    k = m = 0
    for e in prof.events():
        if str(e.device_type).endswith('CUDA'):
            if e.name.startswith(('Memcpy', 'Memset')): m += 1
            else: k += 1
    return k, m
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(2): step()
    torch.cuda.synchronize()
k_step, m_step = kernels(prof)
# the loss alone: leaf maps -> loss -> backward to the maps (moment box and its backward included)
with torch.no_grad():
    feats = model.extract_feat(batch['img'])
    outs = model.bbox_head(feats, batch['img_meta'])
leaves = [[t.detach().clone().requires_grad_() for t in group] for group in outs]
def loss_only():
    losses = model.bbox_head.loss(*leaves, batch['gt_bboxes'], batch['gt_labels'], batch['gt_keypoints'], batch['img_meta'], cfg.train_cfg)
    sum(sum(v) for v in losses.values()).backward()
for _ in range(2): loss_only()
torch.cuda.synchronize()
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    t0 = time.time()
    for _ in range(2): loss_only()
    t1 = time.time()
    torch.cuda.synchronize()
k_loss, m_loss = kernels(prof)
print(json.dumps(dict(tree=ROOT, fused=os.environ.get('KGDET_FUSED_SERIAL_LOSS', '1'), step_ms_median=round(ts[2][0], 3),
                      step_ms_all=[round(a, 3) for a, _ in ts], enqueue_ms_median=round(sorted(b for _, b in ts)[2], 3),
                      kernels_per_step=k_step / 2, copies_per_step=m_step / 2, loss_kernels=k_loss / 2, loss_copies=m_loss / 2,
                      loss_host_ms_under_profiler=round((t1 - t0) / 2 * 1e3, 2))), flush=True)
