#!/usr/bin/env python3
"""`python predict.py [-model state_dict.pth] image` — the reference's predict.py (predict.py:30-72 there) on the MI355X path:
load the checkpoint (the reference's `MaskRCNN.state_dict()` key layout loads unchanged), read the image, run
`MaskRCNNInference.detect` — resize + pad + mean-subtract, ResNet-101-FPN trunk, RPN, proposal NMS, RoIAlign, heads, per-class
NMS, mask head, full-size mask pasting, all on the GPU with one host synchronisation — and print one line per detection
(class id, COCO class name, box, score), as the reference does. Its matplotlib window (`utils.display_instances`) is out of
scope; `--save out.npz` stores class ids, scores, boxes and the full-size boolean masks instead, and `--render out.png` writes
the picture the reference's deterministic renderer (`data.blend_image`) draws: masks, outlines and boxes composited on the GPU
(`image.blend_image`), one [H,W,3] copy to the host, the labels drawn there with PIL.

The reference's weights (models/mask_rcnn_coco.pth, a manual download) are not available offline: without `-model` the script
refuses to guess, and `--random-weights` runs the same path on seeded random weights of the same architecture (plumbing /
timing runs; the detections mean nothing).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MS-COCO's 80 category names in the order of the class ids 1..80 the COCO-trained checkpoint predicts (0 = background)
COCO_NAMES = (
    'BG', 'person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat', 'traffic light',
    'fire hydrant', 'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant',
    'bear', 'zebra', 'giraffe', 'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard',
    'sports ball', 'kite', 'baseball bat', 'baseball glove', 'skateboard', 'surfboard', 'tennis racket', 'bottle',
    'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl', 'banana', 'apple', 'sandwich', 'orange', 'broccoli',
    'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair', 'couch', 'potted plant', 'bed', 'dining table', 'toilet',
    'tv', 'laptop', 'mouse', 'remote', 'keyboard', 'cell phone', 'microwave', 'oven', 'toaster', 'sink',
    'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear', 'hair drier', 'toothbrush',
)


def read_image(path):
    """RGB uint8 [h, w, 3] (skimage.io.imread + grey2rgb in the reference, predict.py:57-59)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)   # a writable copy


def main(argv=None):
    ap = argparse.ArgumentParser(description="Mask RCNN Predictor (MI355X path)")
    ap.add_argument("-model", type=str, default=None, help="trained model: a torch.save()d state_dict of the reference's MaskRCNN")
    ap.add_argument("--random-weights", action="store_true", help="seeded random weights instead of a checkpoint (plumbing runs)")
    ap.add_argument("--backbone", default="resnet101", choices=["resnet50", "resnet101"], help="the reference hard-codes resnet101")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f32+f16x3", "f16"])
    ap.add_argument("--save", default=None, help="write class_ids / scores / boxes / masks to this .npz")
    ap.add_argument("--coco-json", default=None, help="write COCO result records (image_id, category_id, bbox, score, "
                                                     "segmentation as RLE: build_coco_results, coco.py:53-60) to this file; score it with "
                                                     "`python -m maskrcnn_amd.cocoeval GT.json FILE`")
    ap.add_argument("--render", default=None, metavar="FILE",
                    help="write the image with every instance's mask, outline, box and label on it (data.blend_image) to this file; "
                         "the format follows the extension")
    ap.add_argument("--seed", type=int, default=None, help="random.seed(K) before the instance colours of --render are drawn")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("image", type=str, help="image file")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("predict.py needs a GPU (the product has no CPU path)")
    from maskrcnn_amd import modules
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import MaskRCNNInference

    if args.model:
        sd = torch.load(args.model, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    elif args.random_weights:
        sd = modules.synthetic_state_dict(args.backbone)
    else:
        raise SystemExit("predict.py: give -model <state_dict.pth> (the reference's models/mask_rcnn_coco.pth) or --random-weights")
    cfg = InferenceConfig(backbone=args.backbone)          # CocoInferenceConfig: 1024 x 1024 canvas, 500 proposals, 50 detections
    net = MaskRCNNInference(sd, cfg, args.device, precision=args.precision)
    img = read_image(args.image)
    class_ids, scores, boxes, masks = net.detect([img])[0]
    out = []
    if class_ids is not None:
        ids, sc, bx = class_ids.tolist(), scores.tolist(), boxes.tolist()
        for j, b, s in zip(ids, bx, sc):
            name = COCO_NAMES[j] if 0 <= j < len(COCO_NAMES) else "?"
            print(j, name, [int(v) for v in b], round(float(s), 6))
            out.append((j, name, b, s))
    else:
        print("no instances")
    if args.save:
        import numpy as np
        if class_ids is None:
            np.savez_compressed(args.save, class_ids=np.zeros(0, np.int64), scores=np.zeros(0, np.float32),
                                boxes=np.zeros((0, 4), np.float32), masks=np.zeros((0,) + img.shape[:2], bool))
        else:
            np.savez_compressed(args.save, class_ids=class_ids.cpu().numpy(), scores=scores.cpu().numpy(),
                                boxes=boxes.cpu().numpy(), masks=masks.cpu().numpy())
    if args.coco_json:
        import json
        from maskrcnn_amd import image as imagelib
        records = []
        if class_ids is not None:
            # the masks the lines above came with, encoded on the device (grey levels when the image was resized: > 127)
            rle = imagelib.rle_masks(masks, 0 if masks.dtype == torch.bool else 127)
            image_id = os.path.splitext(os.path.basename(args.image))[0]
            for (j, _, b, s), seg in zip(out, rle.to_coco()):
                y1, x1, y2, x2 = b
                records.append({"image_id": image_id, "category_id": j,
                                "bbox": [round(x1, 1), round(y1, 1), round(x2 - x1, 1), round(y2 - y1, 1)], "score": s,
                                "segmentation": {"size": seg["size"], "counts": seg["counts"].decode("ascii")}})
        with open(args.coco_json, "w") as fh:
            json.dump(records, fh)
    if args.render:
        render(args.render, img, out, boxes, masks, args.seed, args.device)
    return out


def render(path, img, detections, boxes, masks, seed=None, device="cuda:0"):
    """data.blend_image(image, names, boxes, masks, scores) into a file: the device tensors detect() returned go through
    image.blend_image as they are (no dense mask leaves the device), the rendered [H,W,3] image comes to the host once, and the
    labels are drawn there as data.py:398-401 does. Unlike the reference, a later rectangle cannot overdraw an earlier label."""
    import random
    from PIL import Image, ImageDraw
    from maskrcnn_amd import image as imagelib
    if not detections:                                      # blend_image returns the image as it is (data.py:385-387)
        Image.fromarray(img).save(path)
        return
    if seed is not None:
        random.seed(seed)
    colors = imagelib.random_colors(len(detections))
    fusion = Image.fromarray(imagelib.blend_image(img, boxes, masks, colors, device=device).cpu().numpy())
    draw = ImageDraw.Draw(fusion)
    for (_, name, b, s), color in zip(detections, colors):
        draw.text((b[1], b[0]), name + " {:.3f}".format(s), color)
    fusion.save(path)


if __name__ == "__main__":
    main()
