"""Cases shared by tests/test_rpn_train_host.py and tests/test_gpu_rpn_train.py: the pyramids, the index sets, the data and the stock-torch
float64 graphs the RPN's training branch is checked against. Everything here is CPU code; nothing imports the library.

The pyramid is the smallest on which each mechanism can go wrong: non-square 6x5, 3x3, a 2x1 level and two 1x1 levels (eight of nine
taps are padding there), three anchors per location. The index sets hold corners and borders, two and three anchors on one pixel,
horizontally, vertically and diagonally adjacent pixels (overlapping footprints), entries on both sides of a level boundary, an image
without an entry, one at capacity and one over it."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

SIZES = [(6, 5), (3, 3), (2, 1), (1, 1), (1, 1)]
APL = 3
BATCH = 2
FIRST = [0, 90, 117, 123, 126, 129]           # the first anchor of each level, and A
A = FIRST[-1]
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


def anchor(level, y, x, r):
    return FIRST[level] + (y * SIZES[level][1] + x) * APL + r


Case = collections.namedtuple("Case", "id capacity anchors channels hidden")   # anchors: one ascending list per image

_CORNERS = [anchor(0, 0, 0, 0), anchor(0, 0, 4, 1), anchor(0, 5, 0, 2), anchor(0, 5, 4, 2),      # the four corners; 89 ends level 0
            anchor(1, 0, 0, 0), anchor(1, 2, 2, 2), anchor(2, 0, 0, 0), anchor(4, 0, 0, 0)]      # 90 starts level 1; 2x1 and 1x1 levels
_OVERLAP = [anchor(0, 0, 2, 1), anchor(0, 2, 2, 0), anchor(0, 2, 2, 2), anchor(0, 2, 3, 1),      # a border; two on one pixel; horizontal
            anchor(0, 3, 2, 0), anchor(0, 3, 3, 0), anchor(0, 3, 3, 1), anchor(0, 3, 3, 2)]      # vertical; diagonal, three on one pixel
_OVER = [1, 4, 30, 31, 44, 88, 89, 90, 91, 118, 122, 128]                                        # twelve: four over a capacity of 8
CASES = [
    Case("corners_and_empty", 8, (_CORNERS, []), 8, 32),                  # image 0 at capacity, image 1 with num = 0
    Case("overlap_and_over", 8, (_OVERLAP, _OVER), 8, 32),                # image 1 over capacity: the first 8 are kept
    Case("wide_k128", 128, (list(range(0, A, 2)), list(range(A))), 8, 32),   # 65 entries; all 129 anchors, one over 128
    Case("corners_c256", 8, (_CORNERS, _OVERLAP[:5] + [anchor(3, 0, 0, 1)]), 256, 512),   # the model's widths
]


def case(name):
    return next(c for c in CASES if c.id == name)


def match_of(c) -> np.ndarray:
    """int32 [B,A]: the listed anchors alternately +1 and -1 (the first one positive), every other anchor 0."""
    m = np.zeros((BATCH, A), np.int32)
    for b, listed in enumerate(c.anchors):
        m[b, listed] = np.where(np.arange(len(listed)) % 2 == 0, 1, -1)
    return m


def kept_match(c) -> np.ndarray:
    """match_of(c) with the anchors past the capacity set to 0: what the branch computes on when an image overflows."""
    m = match_of(c)
    for b, listed in enumerate(c.anchors):
        m[b, listed[c.capacity:]] = 0
    return m


def rng(seed):
    return torch.Generator().manual_seed(seed)


def rounded_maps(c, seed=0):
    """float32 NHWC maps of unit scale with -0 planted in each (a copy must keep its sign)."""
    g = rng(seed)
    maps = [torch.randn(BATCH, h, w, c.channels, generator=g) for h, w in SIZES]
    for m in maps:
        m[:, 0, 0, 0] = -0.0
        m[:, -1, -1, -1] = -0.0
    return maps


def integer_maps(c, seed=1, bound=2):
    g = rng(seed)
    return [torch.randint(-bound, bound + 1, (BATCH, h, w, c.channels), generator=g).to(F32) for h, w in SIZES]


def dpatch_of(c, integer, seed=2):
    g = rng(seed)
    shape = (BATCH * c.capacity, 9 * c.channels)
    return torch.randint(-8, 9, shape, generator=g).to(F32) if integer else torch.randn(shape, generator=g)


# ------------------------------------------------------------------------------------------------------- stock torch, float64
def unfold_patches(maps, index, num):
    """The gather as F.unfold on the padded map: maps [B,H,W,C] (any float dtype) → [B*K,9*C] in (ky, kx, c) order."""
    index, num = np.asarray(index), np.asarray(num)
    b, k = index.shape
    c = maps[0].shape[3]
    out = torch.zeros(b, k, 9 * c, dtype=maps[0].dtype)
    for l, m in enumerate(maps):
        h, w = m.shape[1:3]
        cols = F.unfold(m.permute(0, 3, 1, 2), kernel_size=3, padding=1)              # [B, C*9, H*W], rows (c, ky, kx)
        cols = cols.view(b, c, 9, h * w).permute(0, 3, 2, 1).reshape(b, h * w, 9 * c)  # [B, H*W, (ky, kx, c)]
        for i in range(b):
            for s in range(int(num[i])):
                a = int(index[i, s])
                if FIRST[l] <= a < FIRST[l + 1]:
                    out[i, s] = cols[i, (a - FIRST[l]) // APL]
    return out.view(b * k, 9 * c)


def unfold_scatter(dpatch, index, num, channels):
    """The scatter as the autograd of unfold_patches, in float64 → [grad_l float64 [B,H_l,W_l,C]]."""
    maps = [torch.zeros(BATCH, h, w, channels, dtype=F64, requires_grad=True) for h, w in SIZES]
    (unfold_patches(maps, index, num) * dpatch.to(F64)).sum().backward()
    return [torch.zeros_like(m) if m.grad is None else m.grad for m in maps]     # None: no entry on that level


Params = collections.namedtuple("Params", "shared_w shared_b class_w class_b bbox_w bbox_b")   # the reference's OIHW layouts


def integer_params(c, seed=3):
    """Weights in {-1, 0, 1} and biases in {-2 .. 2}, float32."""
    g = rng(seed)
    r = lambda *shape, bound=1: torch.randint(-bound, bound + 1, shape, generator=g).to(F32)
    return Params(r(c.hidden, c.channels, 3, 3), r(c.hidden, bound=2), r(2 * APL, c.hidden, 1, 1), r(2 * APL, bound=2),
                  r(4 * APL, c.hidden, 1, 1), r(4 * APL, bound=2))


def rounded_params(c, seed=4):
    g = rng(seed)
    n = lambda *shape, scale: torch.randn(shape, generator=g) * scale
    k = 9 * c.channels
    return Params(n(c.hidden, c.channels, 3, 3, scale=k ** -0.5), n(c.hidden, scale=0.5), n(2 * APL, c.hidden, 1, 1, scale=c.hidden ** -0.5),
                  n(2 * APL, scale=0.5), n(4 * APL, c.hidden, 1, 1, scale=c.hidden ** -0.5), n(4 * APL, scale=0.5))


def state_dict_of(p: Params, prefix="rpn."):
    names = ("conv_shared.weight", "conv_shared.bias", "conv_class.weight", "conv_class.bias", "conv_bbox.weight", "conv_bbox.bias")
    return {prefix + n: v.clone() for n, v in zip(names, p)}


def dense_graph(maps, p, dtype=F64, relu=True):
    """The stock-torch dense RPN on whole maps: F.conv2d with padding 1, ReLU, the two 1x1 heads → (logits [B,A,2], bbox [B,A,4],
    pre: the shared conv's pre-activations per level [B,hidden,H,W]). maps and p are used as they are given (leaves of the caller)."""
    logits, bbox, pre = [], [], []
    for m in maps:
        z = F.conv2d(m.to(dtype).permute(0, 3, 1, 2), p.shared_w.to(dtype), p.shared_b.to(dtype), padding=1)
        pre.append(z)
        h = torch.relu(z) if relu else z
        b = m.size(0)
        logits.append(F.conv2d(h, p.class_w.to(dtype), p.class_b.to(dtype)).permute(0, 2, 3, 1).reshape(b, -1, 2))
        bbox.append(F.conv2d(h, p.bbox_w.to(dtype), p.bbox_b.to(dtype)).permute(0, 2, 3, 1).reshape(b, -1, 4))
    return torch.cat(logits, 1), torch.cat(bbox, 1), pre


def leaves(maps, p, dtype=F64):
    """Fresh leaves of the maps and the six parameters in dtype, each requiring a gradient."""
    maps = [m.detach().to(dtype).clone().requires_grad_(True) for m in maps]
    return maps, Params(*[v.detach().to(dtype).clone().requires_grad_(True) for v in p])


def sampled_rows(full, index, num):
    """full [B,A,n] → [B,K,n]: row index[b,k] for k < num[b], zeros for the empty slots (differentiable)."""
    index = torch.as_tensor(np.asarray(index)).to(torch.int64)
    live = (torch.arange(index.size(1))[None, :] < torch.as_tensor(np.asarray(num)).to(torch.int64)[:, None])
    rows = full.gather(1, index.clamp(min=0)[:, :, None].expand(-1, -1, full.size(2)))
    return rows * live[:, :, None].to(full.dtype)


def upstream(c, seed=5):
    """An integer upstream gradient on (logits [B,K,2], bbox [B,K,4]), float32."""
    g = rng(seed)
    return (torch.randint(-3, 4, (BATCH, c.capacity, 2), generator=g).to(F32), torch.randint(-3, 4, (BATCH, c.capacity, 4), generator=g).to(F32))


def exact_reference(c, maps, p, index, num, gl, gb):
    """Outputs and gradients of the dense float64 graph read at the sampled anchors, the upstream gradient injected at the live
    slots → (logits [B,K,2], bbox [B,K,4], [map gradients], Params of gradients), all float64."""
    m64, p64 = leaves(maps, p)
    logits, bbox, _ = dense_graph(m64, p64)
    lo, bo = sampled_rows(logits, index, num), sampled_rows(bbox, index, num)
    ((lo * gl.to(F64)).sum() + (bo * gb.to(F64)).sum()).backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    return lo.detach(), bo.detach(), [zero(m) for m in m64], Params(*[zero(v) for v in p64])


def exactness_bound(c, maps, p, index, num, gl, gb) -> float:
    """The largest sum of ABSOLUTE terms anywhere in that graph, forward and backward: the same graph on |maps| and |parameters| without
    the ReLU's cut, with |upstream|. No partial sum of the real graph, in any order, exceeds it."""
    a = lambda v: v.abs()
    m64, p64 = leaves([a(m) for m in maps], Params(*[a(v) for v in p]))
    logits, bbox, pre = dense_graph(m64, p64, relu=False)
    for z in pre:
        z.retain_grad()
    lo, bo = sampled_rows(logits, index, num), sampled_rows(bbox, index, num)
    ((lo * a(gl).to(F64)).sum() + (bo * a(gb).to(F64)).sum()).backward()
    values = [logits, bbox, *pre, *[z.grad for z in pre if z.grad is not None], *[m.grad for m in m64], *[v.grad for v in p64]]
    return max(float(v.detach().abs().max()) for v in values)


def target_bbox_of(c, seed=6):
    return torch.randn(BATCH, c.capacity, 4, generator=rng(seed)) * 0.5


def stock_losses(maps, p, match, target_bbox):
    """RPN.class_loss and RPN.boxes_loss on the concatenation of the batch (reduction "mean"), float64, from the dense graph:
    torch.nonzero, gathers, F.cross_entropy and F.smooth_l1_loss → (class loss, box loss, maps, parameters: the leaves), with the
    gradients of class + box in the leaves' .grad."""
    m64, p64 = leaves(maps, p)
    logits, bbox, _ = dense_graph(m64, p64)
    match = torch.as_tensor(match)
    nz = torch.nonzero(match != 0)
    cls = F.cross_entropy(logits[nz[:, 0], nz[:, 1]], (match[nz[:, 0], nz[:, 1]] == 1).to(torch.int64))
    rows, targets = [], []
    for b in range(match.size(0)):
        pos = torch.nonzero(match[b] == 1)[:, 0][:target_bbox.size(1)]
        rows.append(bbox[b, pos])
        targets.append(target_bbox[b, :len(pos)].to(F64))
    box = F.smooth_l1_loss(torch.cat(rows), torch.cat(targets))
    (cls + box).backward()
    return cls.detach(), box.detach(), m64, p64


def sampled_pre_activations(maps, p, index, num) -> torch.Tensor:
    """The shared conv's pre-activations at the sampled pixels, float64 [entries, hidden]."""
    _, _, pre = dense_graph([m.to(F64) for m in maps], Params(*[v.to(F64) for v in p]))
    index, num = np.asarray(index), np.asarray(num)
    rows = []
    for b in range(index.shape[0]):
        for k in range(int(num[b])):
            a = int(index[b, k])
            l = max(i for i in range(len(SIZES)) if a >= FIRST[i])
            pix = (a - FIRST[l]) // APL
            rows.append(pre[l][b, :, pix // SIZES[l][1], pix % SIZES[l][1]])
    return torch.stack(rows)


def relu_margin(maps, p, index, num) -> float:
    """The smallest |pre-activation| of the shared conv at a sampled pixel, in float64."""
    return float(sampled_pre_activations(maps, p, index, num).abs().min())


def separated_params(c, maps, index, num, margin=2e-3):
    """rounded_params(c) with the shared conv's bias moved, channel by channel and in steps of 2 * margin, to the first value that
    leaves every sampled pre-activation of the channel at least `margin` from 0: a ReLU flip between the routes is then not a
    rounding question. tests/test_rpn_train_host.py asserts the outcome in float64."""
    p = rounded_params(c)
    z = sampled_pre_activations(maps, p, index, num)
    bias = p.shared_b.clone()
    for j in range(c.hidden):
        step = next(t for t in range(1000) if float((z[:, j] + 2 * margin * t).abs().min()) >= margin)
        bias[j] += 2 * margin * step
    return p._replace(shared_b=bias)
