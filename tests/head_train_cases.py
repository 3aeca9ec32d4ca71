"""Cases shared by tests/test_head_train_host.py and tests/test_gpu_head_train.py: the target tables, the data and the stock-torch
float64 graphs the heads' training mode is checked against. Everything here is CPU code; nothing imports the library.

The class-plane ops: B = 2 images of count = 8 slots with P = 3 plane slots. The tables hold an image with num = 0, an image with all P
slots active, two slots of one class in one image and across images, class C - 1, a class without a slot, a negative among the first P,
an id >= C and a negative id below num (status bit 1), a positive at slot P (status bit 2). Planes are 4 x 4 (one partial chunk of the 64
pixel chunks), 9 x 9 (two chunks: 64 + 17) and 17 x 17 (five chunks, and two passes of the loss kernels' 256 threads); Cin is 8, 256 (one
full group of 64 lanes x 4 channels) and 320 (a second, partial group).

The whole head: a 16 / 8 / 4 / 2 pyramid of 8 channels, 5 classes, pool 2 (so 4 x 4 planes), a hidden width of 32."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

BATCH, COUNT, SLOTS = 2, 8, 3
F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
BAD, NO_ROOM = 2, 4

Case = collections.namedtuple("Case", "id ids num cin classes side status")
CASES = [
    # image 0 has num = 0 (its ids are whatever a padding slot holds); image 1 has all P slots active, class C - 1 among them
    Case("empty_and_full", ([3, 1, 2, 1, 0, 0, 0, 0], [1, 2, 4, 0, 0, 0, 0, 0]), (0, 6), 8, 5, 4, (0, 0)),
    # class 2 twice in image 0 and once in image 1; classes 1 and 3 without a slot; a negative among the first P of image 1
    Case("shared_class", ([2, 2, 4, 0, 0, 0, 0, 0], [2, 0, 4, 0, 0, 0, 0, 0]), (4, 3), 8, 5, 4, (0, 0)),
    # image 0: an id of C and a negative id below num (bit 1), a positive at slot P below num (bit 2); image 1: slot 2 is past num
    Case("bad_and_no_room", ([5, -1, 1, 2, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0, 0]), (5, 2), 8, 5, 4, (BAD | NO_ROOM, 0)),
    Case("model_widths", ([80, 17, 80, 0, 0, 0, 0, 0], [17, 1, 0, 0, 0, 0, 0, 0]), (3, 8), 256, 81, 4, (0, 0)),
    Case("two_chunks", ([1, 4, 1, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0, 0, 0]), (3, 1), 320, 5, 9, (0, 0)),
    Case("five_chunks", ([3, 3, 0, 0, 0, 0, 0, 0], [0, 3, 0, 0, 0, 0, 0, 0]), (2, 2), 8, 5, 17, (0, 0)),
]
NAMES = [c.id for c in CASES]


def case(name):
    return next(c for c in CASES if c.id == name)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def ids_of(c):
    return np.array(c.ids, np.int32), np.array(c.num, np.int32)


def active(c):
    """(bool [B,P], class [B,P]) from the case's own definition."""
    ids, num = ids_of(c)
    on = np.zeros((BATCH, SLOTS), bool)
    for b in range(BATCH):
        for s in range(SLOTS):
            on[b, s] = s < min(num[b], SLOTS) and 0 < ids[b, s] < c.classes
    return on, ids[:, :SLOTS].astype(np.int64)


Operands = collections.namedtuple("Operands", "x w bias dy target")


def operands(c, integer: bool, seed=0) -> Operands:
    """x [B*P,side,side,Cin], w [C,Cin], bias [C], dy [B*P,side,side], target_mask [B,count,side,side] (0 / 1), float32. integer: x in
    -4 .. 4, w in {-1, 0, 1}, bias and dy integers; else rounded values of unit scale."""
    g = rng(100 + seed)
    s, q = BATCH * SLOTS, c.side
    if integer:
        r = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        x, w, bias, dy = r(-4, 4, s, q, q, c.cin), r(-1, 1, c.classes, c.cin), r(-3, 3, c.classes), r(-5, 5, s, q, q)
    else:
        n = lambda *shape: torch.randn(shape, generator=g)
        x, w, bias, dy = n(s, q, q, c.cin), n(c.classes, c.cin) * c.cin ** -0.5, n(c.classes) * 0.5, n(s, q, q)
    target = (torch.rand(BATCH, COUNT, q, q, generator=g) < 0.5).to(F32)
    return Operands(x, w, bias, dy, target)


def poisoned(c, t: torch.Tensor, per_count: bool = False) -> torch.Tensor:
    """t with NaN in the rows of the slots that are not active: [B*P,...] / [B,P,...], or [B,count,...] with per_count (there every slot
    at or past P is poisoned too)."""
    on, _ = active(c)
    out = t.clone()
    v = out.view(BATCH, COUNT if per_count else SLOTS, *t.shape[(2 if t.size(0) == BATCH else 1):])
    for b in range(BATCH):
        for s in range(v.size(1)):
            if s >= SLOTS or not on[b, s]:
                v[b, s] = float("nan")
    return out


def dense_conv_reference(c, o: Operands, act: int):
    """The dense stock graph in float64: F.conv2d to all C planes (sigmoid at act 2), the class plane of every active slot, the upstream
    gradient dy injected there → (y [B*P,side,side] with zeros for the other slots, dx, dw [C,Cin], dbias [C]), float64."""
    on, k = active(c)
    x, w, bias = (v.to(F64).clone().requires_grad_(True) for v in (o.x, o.w, o.bias))
    z = F.conv2d(x.permute(0, 3, 1, 2), w[:, :, None, None], bias)
    planes = torch.sigmoid(z) if act == 2 else z
    rows = [planes[i, int(k.reshape(-1)[i])] if on.reshape(-1)[i] else torch.zeros(c.side, c.side, dtype=F64) for i in range(BATCH * SLOTS)]
    y = torch.stack(rows)
    (y * o.dy.to(F64)).sum().backward()
    return y.detach(), x.grad, w.grad, bias.grad


def conv_exactness_bound(c, o: Operands) -> float:
    """The largest sum of absolute terms anywhere in that graph at act 0, forward and backward: no partial sum, in any order, exceeds it."""
    on, _ = active(c)
    live = torch.from_numpy(on.reshape(-1)).to(F64)[:, None, None]
    x, w, bias, dy = (v.to(F64).abs() for v in (o.x, o.w, o.bias, o.dy))
    z = torch.einsum("sijc,kc->skij", x, w) + bias[None, :, None, None]
    dyl = dy * live
    dw = torch.einsum("sij,sijc->c", dyl, x)            # every class's row is below the sum over all slots
    return max(float(z.max()), float(dw.max()), float(dyl.sum()), float((dyl[..., None] * w.max()).max()))


def dense_bce_reference(c, p: torch.Tensor, target: torch.Tensor, reduction: str):
    """F.binary_cross_entropy in float64 on the class planes of the active slots ("mean": over the batch's concatenation; "per_image") →
    (loss float64 0-dim or [B], grad float64 [B,P,side,side] for an upstream gradient of 1 on every loss). An empty loss is 0."""
    on, _ = active(c)
    p64 = p.to(F64).clone().requires_grad_(True)
    per_image = []
    for b in range(BATCH):
        rows = [s for s in range(SLOTS) if on[b, s]]
        per_image.append((torch.stack([p64[b, s] for s in rows]), torch.stack([target[b, s].to(F64) for s in rows])) if rows else None)
    live = [v for v in per_image if v is not None]
    zero = p64.sum() * 0
    if reduction == "mean":
        loss = F.binary_cross_entropy(torch.cat([v[0] for v in live]), torch.cat([v[1] for v in live])) if live else zero
    else:
        loss = torch.stack([F.binary_cross_entropy(*v) if v is not None else zero for v in per_image])
    loss.sum().backward()
    return loss.detach(), p64.grad


def probabilities(c, seed=1) -> torch.Tensor:
    """p float32 [B,P,side,side] in (1e-3, 1 - 1e-3)."""
    return (torch.rand(BATCH, SLOTS, c.side, c.side, generator=rng(200 + seed)) * 0.998 + 0.001).to(F32)


# ------------------------------------------------------------------------------------------------------------------ whole head
HEAD_SIZES = [(16, 16), (8, 8), (4, 4), (2, 2)]
DEPTH, HIDDEN, CLASSES, POOL, AREA = 8, 32, 5, 2, 1024.0 * 1024.0
EPS = 1e-3
_SIDE = {l: 2.0 ** (l - 4.0) * 224.0 / 1024.0 for l in (2, 3, 4, 5)}      # a square box in the middle of level l's range

HeadCase = collections.namedtuple("HeadCase", "id ids num_pos num_neg")
HEAD_CASES = [
    HeadCase("full_and_one", ([1, 4, 1, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0]), (3, 1), (3, 2)),
    HeadCase("two_and_empty", ([3, 3, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]), (2, 0), (4, 0)),
]
HEAD_NAMES = [h.id for h in HEAD_CASES]


def head_case(name):
    return next(h for h in HEAD_CASES if h.id == name)


def head_rois(seed=0) -> torch.Tensor:
    """float32 [B,count,4] normalised (y1, x1, y2, x2): square boxes in the middle of the levels 2 .. 5, two per level, well inside."""
    g = rng(300 + seed)
    rois = torch.zeros(BATCH, COUNT, 4)
    for b in range(BATCH):
        for s in range(COUNT):
            side = _SIDE[2 + (s + b) % 4] * (1.0 + 0.2 * (float(torch.rand(1, generator=g)) - 0.5))
            cy, cx = (0.3 + 0.4 * torch.rand(2, generator=g)).tolist()
            rois[b, s] = torch.tensor([cy - side / 2, cx - side / 2, cy + side / 2, cx + side / 2])
    return rois


def head_levels(rois) -> np.ndarray:
    r = rois.to(F64).reshape(-1, 4).numpy()
    k = 4.0 + np.log2(np.sqrt((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])) / (224.0 / np.sqrt(AREA)))
    assert np.abs(k[:, None] - np.array([2.5, 3.5, 4.5])[None]).min() > 0.1, "a box near a level boundary"
    return np.clip(np.rint(k), 2, 5).astype(np.int64)


def head_targets(h, seed=0):
    """dict of CPU tensors: rois, ids int32 [B,count], num_pos, num_neg int32 [B], deltas [B,count,4], mask [B,count,4,4] (0 / 1; zeros past
    the positives, as detection_targets writes them)."""
    g = rng(400 + seed)
    ids = torch.tensor(h.ids, dtype=I32)
    num_pos, num_neg = torch.tensor(h.num_pos, dtype=I32), torch.tensor(h.num_neg, dtype=I32)
    deltas = torch.randn(BATCH, COUNT, 4, generator=g) * 0.5
    mask = (torch.rand(BATCH, COUNT, 2 * POOL, 2 * POOL, generator=g) < 0.5).to(F32)
    for b in range(BATCH):
        deltas[b, int(num_pos[b]):], mask[b, int(num_pos[b]):] = 0, 0
    return dict(rois=head_rois(seed), ids=ids, num_pos=num_pos, num_neg=num_neg, deltas=deltas, mask=mask)


def detection_targets_of(t, device="cpu"):
    from maskrcnn_amd.targets import DetectionTargets
    minus = torch.full(tuple(t["ids"].shape), -1, dtype=I32)
    vals = (t["rois"], t["ids"], t["deltas"], t["mask"], minus, minus, t["num_pos"], t["num_neg"], torch.zeros(t["ids"].size(0), dtype=I32))
    return DetectionTargets(*[v.to(device) for v in vals])


def head_maps(seed=0):
    g = rng(500 + seed)
    return [torch.randn(BATCH, hh, ww, DEPTH, generator=g) for hh, ww in HEAD_SIZES]


def head_params(seed=0) -> dict:
    """A state dict with the reference's names (classifier.*, mask.*), float32, rounded values of a scale that keeps activations at unit
    scale."""
    g = rng(600 + seed)
    n = lambda *shape, scale=1.0: torch.randn(shape, generator=g) * scale
    sd = {}

    def bn(name, ch):
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + 0.1 * n(ch), 0.1 * n(ch)
        sd[name + ".running_mean"], sd[name + ".running_var"] = 0.1 * n(ch), 0.5 + torch.rand(ch, generator=g)
        sd[name + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)

    k1 = DEPTH * POOL * POOL
    sd["classifier.conv1.weight"], sd["classifier.conv1.bias"] = n(HIDDEN, DEPTH, POOL, POOL, scale=k1 ** -0.5), 0.1 * n(HIDDEN)
    bn("classifier.bn1", HIDDEN)
    sd["classifier.conv2.weight"], sd["classifier.conv2.bias"] = n(HIDDEN, HIDDEN, 1, 1, scale=HIDDEN ** -0.5), 0.1 * n(HIDDEN)
    bn("classifier.bn2", HIDDEN)
    sd["classifier.linear_class.weight"], sd["classifier.linear_class.bias"] = n(CLASSES, HIDDEN, scale=HIDDEN ** -0.5), 0.1 * n(CLASSES)
    sd["classifier.linear_bbox.weight"], sd["classifier.linear_bbox.bias"] = n(4 * CLASSES, HIDDEN, scale=HIDDEN ** -0.5), 0.1 * n(4 * CLASSES)
    for i in (1, 2, 3, 4):
        sd[f"mask.conv{i}.weight"], sd[f"mask.conv{i}.bias"] = n(DEPTH, DEPTH, 3, 3, scale=(9 * DEPTH) ** -0.5 * 1.4), 0.1 * n(DEPTH)
        bn(f"mask.bn{i}", DEPTH)
    sd["mask.deconv.weight"], sd["mask.deconv.bias"] = n(DEPTH, DEPTH, 2, 2, scale=DEPTH ** -0.5 * 1.4), 0.1 * n(DEPTH)
    sd["mask.conv5.weight"], sd["mask.conv5.bias"] = n(CLASSES, DEPTH, 1, 1, scale=DEPTH ** -0.5), 0.1 * n(CLASSES)
    return sd


TRAINED = [k for k in head_params() if "bn" not in k]                          # BatchNorm is frozen


def crop64(fm, box, pool):
    """crop_and_resize of one box on one map [H,W,C] → [pool,pool,C], differentiable in fm: bilinear, extrapolation 0."""
    hh, ww, _ = fm.shape

    def axis(c1, c2, size):
        pos = c1 * (size - 1) + torch.arange(pool, dtype=fm.dtype) * ((c2 - c1) * (size - 1) / (pool - 1))
        inside = (pos >= 0) & (pos <= size - 1)
        lo = pos.floor().clamp(0, size - 1).long()
        hi = pos.ceil().clamp(0, size - 1).long()
        return lo, hi, pos - lo.to(fm.dtype), inside

    y0, y1, ly, iy = axis(box[0], box[2], hh)
    x0, x1, lx, ix = axis(box[1], box[3], ww)
    lx_, ly_ = lx[None, :, None], ly[:, None, None]
    top = fm[y0][:, x0] * (1 - lx_) + fm[y0][:, x1] * lx_
    bottom = fm[y1][:, x0] * (1 - lx_) + fm[y1][:, x1] * lx_
    out = top * (1 - ly_) + bottom * ly_
    return out * (iy[:, None, None] & ix[None, :, None]).to(fm.dtype)


def pooled64(maps, rois, pool):
    """The pyramid RoIAlign in stock torch: maps [B,H,W,C], rois [B,n,4] → [B*n,pool,pool,C] in the maps' dtype."""
    levels = head_levels(rois)
    b, n = rois.shape[:2]
    return torch.stack([crop64(maps[levels[i * n + s] - 2][i], rois[i, s].to(maps[0].dtype), pool) for i in range(b) for s in range(n)])


def _bn(x, sd, name):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, EPS)


def stock_graph(maps, t, sd, tape=None):
    """The reference's two heads in stock torch on all count slots and C planes, in the dtype of maps and sd → (logits [B*count,C], bbox
    [B*count,C,4], masks [B*count,C,4,4]). tape: a list that receives every ReLU pre-activation."""
    note = (lambda z: tape.append(z)) if tape is not None else (lambda z: None)
    x = pooled64(maps, t["rois"], POOL).permute(0, 3, 1, 2)
    z = _bn(F.conv2d(x, sd["classifier.conv1.weight"], sd["classifier.conv1.bias"]), sd, "classifier.bn1")
    note(z)
    z = _bn(F.conv2d(torch.relu(z), sd["classifier.conv2.weight"], sd["classifier.conv2.bias"]), sd, "classifier.bn2")
    note(z)
    h = torch.relu(z).flatten(1)
    logits = F.linear(h, sd["classifier.linear_class.weight"], sd["classifier.linear_class.bias"])
    bbox = F.linear(h, sd["classifier.linear_bbox.weight"], sd["classifier.linear_bbox.bias"]).view(h.size(0), -1, 4)
    for i in (1, 2, 3, 4):
        z = _bn(F.conv2d(x, sd[f"mask.conv{i}.weight"], sd[f"mask.conv{i}.bias"], padding=1), sd, f"mask.bn{i}")
        note(z)
        x = torch.relu(z)
    z = F.conv_transpose2d(x, sd["mask.deconv.weight"], sd["mask.deconv.bias"], stride=2)
    note(z)
    z5 = F.conv2d(torch.relu(z), sd["mask.conv5.weight"], sd["mask.conv5.bias"])
    if tape is not None:
        tape.append(("conv5", z5))
    return logits, bbox, torch.sigmoid(z5)


def leaves64(maps, sd):
    maps = [m.detach().to(F64).clone().requires_grad_(True) for m in maps]
    sd = {k: (v.detach().to(F64).clone().requires_grad_(k in TRAINED) if v.is_floating_point() else v) for k, v in sd.items()}
    return maps, sd


def used_slots(h, slots=SLOTS):
    """(rows in the class loss, rows in the box loss, rows in the mask loss) as flat indices b * count + s; the mask loss keeps the
    positives among the first `slots` slots."""
    use, pos, mpos = [], [], []
    for b in range(BATCH):
        n = h.num_pos[b] + h.num_neg[b]
        for s in range(n):
            use.append(b * COUNT + s)
            if h.ids[b][s] > 0:
                pos.append(b * COUNT + s)
                if s < slots:
                    mpos.append(b * COUNT + s)
    return use, pos, mpos


def stock_losses(h, maps, t, sd):
    """Classifier.class_loss, Classifier.boxes_loss and Mask.mask_loss (reduction "mean": the batch's concatenation) in float64 from the
    stock graph → (class, box, mask losses, the leaves maps64 and sd64 with the gradients of the sum of the three in .grad)."""
    m64, sd64 = leaves64(maps, sd)
    logits, bbox, masks = stock_graph(m64, t, sd64)
    use, pos, mpos = (torch.tensor(v, dtype=torch.int64) for v in used_slots(h))
    ids = t["ids"].reshape(-1).to(torch.int64)
    cls = F.cross_entropy(logits[use], ids[use])
    box = F.smooth_l1_loss(bbox[pos, ids[pos]], t["deltas"].reshape(-1, 4)[pos].to(F64))
    mask = F.binary_cross_entropy(masks[mpos, ids[mpos]], t["mask"].reshape(-1, 2 * POOL, 2 * POOL)[mpos].to(F64))
    (cls + box + mask).backward()
    return cls.detach(), box.detach(), mask.detach(), m64, sd64


def margins(maps, t, sd):
    """(the smallest |ReLU pre-activation|, the smallest distance of a conv5 probability from 0 or 1) of the stock graph in float64."""
    m64, sd64 = leaves64(maps, sd)
    tape = []
    with torch.no_grad():
        stock_graph(m64, t, sd64, tape)
    relu = min(float(z.abs().min()) for z in tape if not isinstance(z, tuple))
    p = torch.sigmoid(next(z[1] for z in tape if isinstance(z, tuple)))
    return relu, float(torch.minimum(p, 1 - p).min())


_SHIFTED = ["classifier.bn1.bias", "classifier.bn2.bias", "mask.bn1.bias", "mask.bn2.bias", "mask.bn3.bias", "mask.bn4.bias", "mask.deconv.bias"]


def separated_params(maps, t, margin=2e-3, seed=0) -> dict:
    """head_params() with, layer by layer in graph order, each ReLU layer's additive term (the BatchNorm bias; the deconv's bias) moved
    channel by channel in steps of 2 * margin to the first value that leaves every pre-activation of the channel at least `margin` from 0:
    a ReLU flip between two routes is then not a rounding question. tests/test_head_train_host.py asserts the outcome in float64."""
    sd = head_params(seed)
    for layer, name in enumerate(_SHIFTED):
        m64, sd64 = leaves64(maps, sd)
        tape = []
        with torch.no_grad():
            stock_graph(m64, t, sd64, tape)
        z = [v for v in tape if not isinstance(v, tuple)][layer]
        z = z.transpose(0, 1).flatten(1)                                   # [channels, everything else]
        for j in range(z.size(0)):
            step = next(k for k in range(1000) if float((z[j] + 2 * margin * k).abs().min()) >= margin)
            sd[name][j] += 2 * margin * step
    return sd
