"""The small training helpers scripts written against the reference import from diagan.utils.trainer: AverageMeter, accuracy and
save_np_arr, with the reference's names, arguments and results.  The engine's own loops keep their meters on the device
(models/convnets.py, models/attr_classifier.py) and do not use these."""
import numpy as np
import torch


class AverageMeter:
    """Running weighted mean: update(val, n) adds `val` with weight n; .val is the last value, .avg = .sum / .count."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum = self.sum + val * n
        self.count = self.count + n
        self.avg = self.sum / self.count


def accuracy(output, target, topk=(1,)):
    """Top-k accuracies in percent, one [1] tensor per k: a row counts when its target is among its k largest outputs."""
    with torch.no_grad():
        ranked = output.topk(max(topk), dim=1, largest=True, sorted=True).indices          # [B, maxk]
        hit = ranked.eq(target.view(-1, 1))
        return [hit[:, :k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / target.size(0)) for k in topk]


def save_np_arr(arr, file_path):
    with open(file_path, 'wb') as f:
        np.save(f, arr)
