"""Shared by tests/test_pcl_batch_{cpu,gpu,model_gpu}.py: synthetic images for PCL on image batches, and the batch
definition (include/drn_wsod.h, "PCL refinement on image batches") restated on top of the PER-IMAGE functions of
oracle/pcl_oracle.py, which are imported and not modified.

Definition.  Image i owns rows [img_off[i], img_off[i+1]) and the label vector onehot[i]:
  targets / loss_img[i][b]   what the single-image path gives for image i alone
  loss[b]                    (float32)((sum over i ascending of (float64)loss_img[i][b]) / n)
  dlogits rows of image i    the single-image rows, every entry multiplied once more in float32 by 1.f / (float)n
"""
import numpy as np
import torch

from oracle import pcl_oracle as PO

# The per-branch bounds tests/test_pcl_gpu.py applies (_check_branch, lines 47-61), restated:
#   integers (n_pc, labels, gt_assignment, pc_labels, pc_count, centre rows) and cls_loss_weights: exact  (:49-56)
RTOL_PC = 1e-5        # pc_probs, img_cls_loss_weights: float32 summation order                              (:57-58)
RTOL_LOSS = 1e-5      # |loss - oracle| <= 1e-5 * max(1, |oracle|)                                            (:59)
RTOL_DLOGITS, ATOL_DLOGITS = 2e-4, 1e-8                                                                      # (:61)
RTOL_PROBS, ATOL_PROBS = 2e-6, 1e-9   # device expf softmax against torch's (test_pcl_refine_cascade_vs_oracle, :125)

# (rows per image, K, branches, labelled classes per image: a count, or 0 = an image WITHOUT labels)
CASES = {
    # offsets 40 and 373 are multiples of neither 32 nor 64; unequal R_i; several / one / no labels
    "uneven3": dict(rows=(40, 333, 70), K=20, nb=3, labels=(3, 1, 0)),
    # a single-proposal image, exact word (32) and wave (64 + 1) boundaries
    "edges3": dict(rows=(1, 65, 32), K=5, nb=2, labels=(1, 2, 1)),
    # the per-image maximum next to a tiny image
    "max2": dict(rows=(4096, 33), K=5, nb=2, labels=(2, 1)),
    "four": dict(rows=(50, 64, 31, 97), K=20, nb=2, labels=(1, 0, 3, 2)),
    "eight": dict(rows=(64,) * 8, K=5, nb=3, labels=(1, 2, 1, 3, 1, 2, 0, 1)),
    "one": dict(rows=(333,), K=20, nb=3, labels=(2,)),
}


def make_image(R, K, nb, n_labels, seed):
    """boxes [R,4], WSDDN-shaped scores [R,K], nb logit blocks [R,K+1], labels [K] (the generator of
    tests/test_pcl_gpu.py::test_pcl_refine_cascade_vs_oracle: proposals jittered around a few seed boxes)"""
    rs = np.random.RandomState(1000 + seed)
    W, H = 320.0, 240.0
    nseed = max(2, R // 15)
    sx0, sy0 = rs.rand(nseed) * (W - 80), rs.rand(nseed) * (H - 80)
    sw, sh = 40 + rs.rand(nseed) * (W - sx0 - 40), 40 + rs.rand(nseed) * (H - sy0 - 40)
    pick = rs.randint(0, nseed, size=R)
    jit = rs.randn(R, 4) * 8.0
    x0 = np.clip(sx0[pick] + jit[:, 0], 0, W - 21)
    y0 = np.clip(sy0[pick] + jit[:, 1], 0, H - 21)
    x1 = np.clip(sx0[pick] + sw[pick] + jit[:, 2], x0 + 20, W)
    y1 = np.clip(sy0[pick] + sh[pick] + jit[:, 3], y0 + 20, H)
    boxes = np.stack([x0, y0, x1, y1], 1).astype(np.float32)
    im = np.zeros(K, dtype=np.float32)
    im[rs.permutation(K)[:n_labels]] = 1
    a = torch.from_numpy(rs.randn(R, K).astype(np.float32) * 2.0)
    b = torch.from_numpy(rs.randn(R, K).astype(np.float32) * 3.0)
    last = np.ascontiguousarray((torch.softmax(a, 1) * torch.softmax(b, 0)).numpy())
    logits = [rs.randn(R, K + 1).astype(np.float32) * 2.0 for _ in range(nb)]
    return dict(boxes=boxes, last=last, logits=logits, im=im)


def make_case(name):
    c = CASES[name]
    images = [make_image(R, c["K"], c["nb"], nl, 17 * i + len(name)) for i, (R, nl) in enumerate(zip(c["rows"], c["labels"]))]
    return c, images


def layout(K, nb, pad=3):
    """logit columns like tests/test_pcl_gpu.py::_run: branches neither start at 0 nor touch -> (ld, cols)"""
    return pad + nb * (K + 3), [pad + b * (K + 3) for b in range(nb)]


def image_oracle(img, probs_override=None):
    """the cascade of ONE image through oracle.pcl_oracle.pcl_refine_loss: branch b clusters on branch b-1's softmax
    (probs_override[b]: the probabilities to hand on instead of the oracle's own - the device's, which differ by an ulp).
    -> list over branches of (loss float32, dlogits [R,K+1] float32, probs, targets)"""
    out, prev = [], img["last"]
    for b, lg in enumerate(img["logits"]):
        with np.errstate(all="ignore"):
            loss, dl, probs, t = PO.pcl_refine_loss(lg, img["boxes"], prev, img["im"])
        out.append((np.float32(loss), dl.astype(np.float32), probs, t))
        prev = probs if probs_override is None else probs_override[b]
    return out


def batch_mean(loss_img):
    """loss[b] = (float32)((sum over images, ascending, of (float64)loss_img[i][b]) / n)"""
    loss_img = np.asarray(loss_img, dtype=np.float32)
    n, nb = loss_img.shape
    out = np.zeros(nb, dtype=np.float32)
    for b in range(nb):
        acc = np.float64(0.0)
        for i in range(n):
            acc = acc + np.float64(loss_img[i, b])
        out[b] = np.float32(acc / np.float64(n))
    return out


def scale_rows(dl_single, n):
    """the batch's dlogits rows of an image: the single-image rows times 1.f / (float)n, in float32"""
    return (np.asarray(dl_single, dtype=np.float32) * (np.float32(1.0) / np.float32(n))).astype(np.float32)


def batch_oracle(images, probs_override=None):
    """the definition on a list of images -> dict(per_image=[image_oracle(...)], loss_img [n,nb] float32, loss [nb] float32,
    dlogits = [per image: list over branches of [R_i,K+1] float32])"""
    n = len(images)
    per = [image_oracle(img, None if probs_override is None else probs_override[i]) for i, img in enumerate(images)]
    loss_img = np.array([[br[0] for br in p] for p in per], dtype=np.float32)
    return dict(per_image=per, loss_img=loss_img, loss=batch_mean(loss_img),
                dlogits=[[scale_rows(br[1], n) for br in p] for p in per])
