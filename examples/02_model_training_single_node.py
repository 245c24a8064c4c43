#!/usr/bin/env python3
"""Single-node training from the silver tables.

Equivalent of ``Part 1 .../02_model_training_single_node.py``: load the
train/val tables into memory, build the transfer model (frozen MobileNetV2
base + trainable head), compile Adam + sparse-CE-from-logits + accuracy,
autolog to the tracking store, fit, and log the model.

``--precision bf16`` (or ``auto`` on a GPU) trains on the hand-written
kernels: the images stay uint8 until they are on the device and ``Model``
applies the bf16 policy. The default, ``fp32``, is the plain library path.
"""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import argparse

import numpy as np
import torch

from ddlw_amd.core import setup, tracking
from ddlw_amd.data import read_table
from ddlw_amd.data.decode import decode_resize_u8
from ddlw_amd.data.preprocess import preprocess_batch
from ddlw_amd.models import build_model
from ddlw_amd.train import Model, autolog

IMG_HEIGHT, IMG_WIDTH, IMG_CHANNELS = 64, 64, 3  # synthetic-tree size
BATCH_SIZE = 32
EPOCHS = 3


def load_split(table: str):
    tbl = read_table(table, columns=["content", "label_idx"])
    contents = tbl.column("content").to_pylist()
    labels = tbl.column("label_idx").to_pylist()
    return contents, torch.tensor(labels, dtype=torch.long)


def to_images(contents, img: int, precision: str):
    if precision == "bf16":
        # N x H x W x C bytes; normalization belongs to the model on the device
        return torch.from_numpy(np.stack([decode_resize_u8(c, img, img) for c in contents]))
    return preprocess_batch(contents, img, img)


def batches(xs, ys, bs):
    return [(xs[i : i + bs], ys[i : i + bs]) for i in range(0, len(xs), bs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None)
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--img", type=int, default=IMG_HEIGHT)
    ap.add_argument(
        "--fine-tune-at", type=int, default=None, metavar="K",
        help="also train MobileNetV2 features[K:] (0..23; default: frozen base)",
    )
    ap.add_argument(
        "--precision", choices=("fp32", "bf16", "auto"), default="fp32",
        help="bf16: the fused-kernel path (needs a GPU); auto: bf16 where it works",
    )
    args = ap.parse_args()
    setup(root=args.root)

    train_contents, ys = load_split("silver_train")
    val_contents, vy = load_split("silver_val")
    num_classes = int(ys.max()) + 1

    tracking.set_experiment("single_node_training")
    autolog()
    device = None
    if args.precision != "fp32" and torch.cuda.is_available():
        device = torch.device("cuda:0")
    model = Model(build_model(
        args.img, args.img, IMG_CHANNELS, num_classes,
        fine_tune_at=args.fine_tune_at,
    ), device=device, precision=args.precision)
    xs = to_images(train_contents, args.img, model.precision)
    vx = to_images(val_contents, args.img, model.precision)
    model.compile(optimizer="Adam", learning_rate=1e-3, metrics=("accuracy",))
    with tracking.start_run(run_name="single_node") as run:
        hist = model.fit(
            batches(xs, ys, BATCH_SIZE),
            epochs=args.epochs,
            validation_data=batches(vx, vy, BATCH_SIZE),
        )
        print({k: v[-1] for k, v in hist.history.items()})
        print(f"model logged under runs:/{run.run_id}/model")


if __name__ == "__main__":
    main()
