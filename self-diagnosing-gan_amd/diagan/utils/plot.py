"""LDR scorer front-end (reference: diagan-pkg/diagan/utils/plot.py:220-249).

`calculate_scores` keeps the reference signature and return value (dict of 103 float64 [N]
arrays) but the arithmetic runs in the HIP kernel `diagan_ldr_scores_f64`, which is bit-exact
with the NumPy reference.  `LogitRecord` is the HBM-resident form of the reference's
`logit_results[name]` dict (trainer.py:224,338): snapshots are scattered straight into a device
matrix and never cross PCIe until they are pickled.

Further down, the pictures the reference's scripts draw with this module (plot.py:10-104, 153-174, 269-338): the image panels are
tiled and converted on the device (diagan.utils.image_grid), the bar plot is matplotlib's Agg canvas.  PIL, matplotlib
and the grid binding are imported inside the functions that use them.
"""
import numpy as np
import torch

from diagan import _native as nat

FLOOR = 1e-2     # clip_min lower bound, plot.py:230
RATIO = 50.0     # clip_max_ratio ratio used for every ldr_conf key, plot.py:248


def conf_t_values():
    """The 99 confidence multipliers, exactly as plot.py:247 builds them."""
    return np.arange(0.1, 10.0, 0.1)


def conf_key(t):
    return f'ldr_conf_{t:.1f}_ratio_50'


class LogitRecord:
    """Resident [T_cap, N] logit record (float64 rows = snapshots, columns = dataset index)."""

    def __init__(self, num_data, capacity=64, device='cuda', dtype=torch.float64):
        self.N = int(num_data)
        self.device = torch.device(device)
        self.dtype = dtype
        self.buf = torch.zeros((capacity, self.N), dtype=dtype, device=self.device)
        self.steps = []                       # row r holds snapshot of global step steps[r]
        self._oob = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _grow(self):
        nb = torch.zeros((self.buf.shape[0] * 2, self.N), dtype=self.dtype, device=self.device)
        nb[: self.buf.shape[0]].copy_(self.buf)
        self.buf = nb

    def new_snapshot(self, step):
        """Start the snapshot of `step`; rows start as zeros like np.zeros(N) (trainer.py:144)."""
        if step in self.steps:
            r = self.steps.index(step)
        else:
            if len(self.steps) == self.buf.shape[0]:
                self._grow()
            self.steps.append(step)
            r = len(self.steps) - 1
        self.buf[r].zero_()
        return r

    def scatter(self, row, idx, logit):
        """rec[row, idx] = logit  (trainer.py:154) on the current stream."""
        logit = logit.reshape(-1)
        if logit.dtype != torch.float32:
            logit = logit.float()
        logit = logit.contiguous()
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        if idx.numel() != logit.numel():
            raise RuntimeError(f"scatter: {idx.numel()} indices for {logit.numel()} logits")
        nat.call("diagan_logit_scatter", nat.ptr(logit), nat.ptr(idx), idx.numel(),
                 self.buf[row].data_ptr(), self.N, 1 if self.dtype == torch.float64 else 0,
                 nat.ptr(self._oob), nat.current_stream())

    def check_bounds(self):
        n = int(self._oob.item())
        if n:
            raise IndexError(f"{n} dataset indices were outside [0, {self.N})")

    def to_dict(self):
        """Host dict{step -> float64 ndarray[N]}: the pickle layout of trainer.py:138-140."""
        host = self.buf[: len(self.steps)].to(torch.float64).cpu().numpy()
        return {s: host[r].copy() for r, s in enumerate(self.steps)}

    @classmethod
    def from_dict(cls, logits, device='cuda'):
        steps = list(logits.keys())
        n = len(np.asarray(logits[steps[0]]))
        rec = cls(n, capacity=max(len(steps), 1), device=device)
        host = np.ascontiguousarray(np.stack([np.asarray(logits[s], dtype=np.float64) for s in steps]))
        rec.buf[: len(steps)].copy_(torch.from_numpy(host))
        rec.steps = steps
        return rec

    def window(self, start_epoch, end_epoch):
        """Rows with start <= step < end in insertion order (dict order, plot.py:239)."""
        rows = [r for r, s in enumerate(self.steps) if s >= start_epoch and s < end_epoch]
        if not rows:
            return self.buf[:0]
        if rows == list(range(rows[0], rows[0] + len(rows))):
            return self.buf[rows[0]: rows[0] + len(rows)]       # contiguous view, no copy
        return self.buf[torch.tensor(rows, device=self.device)]


def ldr_scores_device(rec_rows, t_values=None, want_stats=True, exact=True):
    """Run the scorer on a device [T, N] window. Returns (stats dict, conf [n_t, N]) on device."""
    T, N = rec_rows.shape
    if T < 2:
        raise ValueError(f"calculate_scores needs at least 2 snapshots in the window, got {T}")
    if rec_rows.stride(1) != 1:
        rec_rows = rec_rows.contiguous()
    dev = rec_rows.device
    if exact:
        if rec_rows.dtype != torch.float64:
            rec_rows = rec_rows.double()
        dt, fn_name, ws_elt = torch.float64, "diagan_ldr_scores_f64", 8
    else:
        if rec_rows.dtype != torch.float32:
            rec_rows = rec_rows.float()
        dt, fn_name, ws_elt = torch.float32, "diagan_ldr_scores_f32", 4
    tv = conf_t_values() if t_values is None else np.asarray(t_values, dtype=np.float64)
    n_t = len(tv)
    stats = torch.empty((4, N), dtype=dt, device=dev) if want_stats else None
    conf = torch.empty((n_t, N), dtype=dt, device=dev) if n_t else None
    tdev = torch.from_numpy(tv).to(device=dev, dtype=dt) if n_t else None
    ws = torch.empty(max(n_t, 1) * ws_elt, dtype=torch.uint8, device=dev)
    sp = [stats[k].data_ptr() if want_stats else None for k in range(4)]
    nat.call(fn_name, nat.ptr(rec_rows), T, N, rec_rows.stride(0), sp[0], sp[1], sp[2], sp[3],
             nat.ptr(tdev), n_t, nat.ptr(conf), FLOOR, RATIO, nat.ptr(ws), nat.current_stream())
    out = {}
    if want_stats:
        out = {'ldr': stats[0], 'ldrd': stats[1], 'ldrv': stats[2], 'ldrm': stats[3]}
    return out, conf, tv


def calculate_scores(logits, start_epoch=50, end_epoch=75, clip_val=1.5, conf=1, device='cuda',
                     exact=True, keys=None):
    """Drop-in for plot.py:220 -- same keys, float64 ndarray values, window [start, end).

    `logits` is the reference's dict{step -> ndarray[N]} or a resident LogitRecord.
    keys (not in the reference): the scores the caller will read -- the phase-2 command lines consume ONE of the 103
    (train_mimicry_phase2.py:93 `scores[args.resample_score]`); then only the four statistics and the requested
    `ldr_conf_<t>_ratio_50` rows are computed, copied to the host and returned (same values, bit for bit)."""
    rec = logits if isinstance(logits, LogitRecord) else LogitRecord.from_dict(logits, device=device)
    rows = rec.window(start_epoch, end_epoch)
    print(f'calculate_scores -- start_epoch: {start_epoch} end_epoch: {end_epoch} '
          f'logits_arr: {tuple(rows.shape)}')
    t_values = None
    if keys is not None:
        by_key = {conf_key(t): t for t in conf_t_values()}
        unknown = [k for k in keys if k not in by_key and k not in ('ldr', 'ldrd', 'ldrv', 'ldrm')]
        if unknown:
            raise KeyError(f"calculate_scores: unknown score key(s) {unknown}")
        t_values = [by_key[k] for k in keys if k in by_key]
    stats, conf_dev, tv = ldr_scores_device(rows, t_values=t_values, exact=exact)
    score_dict = dict()
    host_stats = torch.stack([stats[k] for k in ('ldr', 'ldrd', 'ldrv', 'ldrm')]).double().cpu().numpy()
    for j, k in enumerate(('ldr', 'ldrd', 'ldrv', 'ldrm')):
        score_dict[k] = host_stats[j]
    if conf_dev is not None:
        host_conf = conf_dev.double().cpu().numpy()
        for j, t in enumerate(tv):
            score_dict[conf_key(t)] = host_conf[j]
    return score_dict


def print_num_params(netG, netD):
    """plot.py helper used by the CLIs (plot.py:107-110; train_mimicry_phase1.py:74)."""
    count = lambda n: n.count_params() if hasattr(n, 'count_params') else sum(p.numel() for p in n.parameters())
    gen_trainable_parameters, disc_trainable_parameters = count(netG), count(netD)
    print(f'gen_trainable_parameters: {gen_trainable_parameters}, '
          f'disc_trainable_parameters: {disc_trainable_parameters}')


# ---- pictures ----------------------------------------------------------------------------------------------------------------
def to_numpy_image(x):
    """[B,C,H,W] in [-1, 1] -> uint8 ndarray [B,H,W,C]: ((x + 1) / 2).clip(0, 1) * 255 in fp32, truncated (plot.py:10-15), converted
    on the device; only the bytes cross to the host."""
    from diagan.utils.image_grid import make_grid_bytes
    B, C, H, W = x.shape
    rows = make_grid_bytes(x, nrow=1, padding=0, conversion="to_numpy_image")          # [B*H, W, 3], one image per grid row
    return rows.reshape(B, H, W, 3)[..., :C].cpu().numpy()


def plot_data(x, num_per_side=10, save_path=None, file_name='plot_data', is_tensor=True, vis=None):
    """The first num_per_side^2 images of x, tiled edge to edge, as save_path/file_name.jpg (plot.py:17-47).  The bytes are those
    the reference tiles -- to_numpy_image of every image, which for a tensor is the grid launch with no padding -- but they are
    written as they are: the reference renders them through a matplotlib figure (imshow + savefig with a tight bounding box),
    which resamples them to the figure's size.  `vis` (a visdom handle there) is accepted and not used."""
    from PIL import Image
    n = num_per_side
    if x.shape[0] < n * n:
        raise IndexError(f"plot_data: {n} x {n} tiles need {n * n} images, got {x.shape[0]}")
    if is_tensor:
        from diagan.utils.image_grid import make_grid_bytes
        img = make_grid_bytes(x[:n * n], nrow=n, padding=0, conversion="to_numpy_image").cpu().numpy()
    else:
        x = np.asarray(x[:n * n], dtype=np.uint8)
        _, h, w, c = x.shape
        img = x.reshape(n, n, h, w, c).transpose(0, 2, 1, 3, 4).reshape(n * h, n * w, c)
        img = np.repeat(img, 3, axis=2) if c == 1 else img
    Image.fromarray(img).save(save_path / f'{file_name}.jpg')


def show_images_grid(x, num_images=25, save_path=None, file_name='show_images_grid', is_tensor=True, vis=None):
    """make_grid(x[:num_images], nrow=10, padding=2, normalize=True) then save_image(grid, normalize=True) as
    save_path/file_name.jpg (plot.py:70-82): the two normalisations are the two passes of the grid launch."""
    from diagan.utils.image_grid import save_image
    assert x.shape[0] >= num_images
    save_image(x[:num_images], save_path / f'{file_name}.jpg', nrow=10, padding=2, normalize=True, passes=2)


def _images_of(dataset, rows):
    """fp32 [len(rows),C,H,W] of a WeightedDataset: one fetch launch when the images are resident, item by item otherwise"""
    inner = getattr(dataset, 'dataset', dataset)
    if hasattr(inner, 'fetch'):
        return inner.fetch(torch.as_tensor(np.ascontiguousarray(rows), dtype=torch.int64))
    return torch.stack([dataset[int(i)][0] for i in rows], 0)


def show_sorted_score_samples(dataset, score, save_path=None, score_name='ae_score', plot_name='ae_score'):
    """The 20 lowest- and the 20 highest-scored training images as {plot_name}_low100.jpg / {plot_name}_high100.jpg
    (plot.py:94-104; the names say 100, the panels hold 20)."""
    sorted_idx = np.argsort(score)
    for range_name, rng in [('low100', sorted_idx[:20]), ('high100', sorted_idx[-20:])]:
        show_images_grid(_images_of(dataset, rng), num_images=20, is_tensor=True, save_path=save_path,
                         file_name=f'{plot_name}_{range_name}')


def _labels_of(dataset):
    inner = getattr(dataset, 'dataset', dataset)
    for name in ('labels', '_targets_host', 'targets'):
        labels = getattr(inner, name, None)
        if labels is not None:
            return np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
    return np.asarray([int(dataset[i][1]) for i in range(len(dataset))])


def plot_score_sort(dataset, score_dict, save_path, phase, plot_metric_name=None):
    """Per score, the bars of up to 5000 randomly chosen ranks of the sorted score, the majority group (label 0) in blue and the
    minority (label 1) in red, as save_path/{phase}_{metric}_sort.jpg (plot.py:153-174).  Takes the reference's draw from
    np.random.  Drawn on an Agg canvas of its own: pyplot is not imported and the global backend is left alone."""
    import matplotlib
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    n_data = len(dataset)
    n_plt = min(5000, n_data)
    plot_idx = np.sort(np.random.choice(n_data, n_plt, replace=False))
    labels = _labels_of(dataset)
    for metric_name, metric in score_dict.items():
        if plot_metric_name and plot_metric_name not in metric_name:
            continue
        print(f'plot_score_sort: {metric_name}')
        metric = np.asarray(metric)
        sorted_idx = np.argsort(metric)[plot_idx]
        sorted_score, sorted_type = metric[sorted_idx], labels[sorted_idx]
        with matplotlib.rc_context({'font.size': 20}):
            fig = Figure(figsize=(16, 8))
            FigureCanvasAgg(fig)
            ax = fig.add_subplot(111)
            ax.set_xlabel('index', fontsize=20)
            ax.set_ylabel(metric_name, fontsize=20)
            for i, color in enumerate(['blue', 'red']):
                ax.bar(np.arange(n_plt)[sorted_type == i], sorted_score[sorted_type == i], color=color)
            fig.savefig(save_path / f'{phase}_{metric_name}_sort.jpg')


def _positive_quarter(images, channel, grid_size):
    """plot.py:279-309 for one channel: per image the count of positive pixels; among the quarter of the images with a positive
    count that have the most, grid_size drawn without replacement (np.random), or None when that quarter is too small"""
    counts = (images[:, channel].reshape(images.shape[0], -1) > 0).sum(-1)
    positive = counts[counts > 0]
    print(torch.quantile(positive.float(), 0.75).item() if positive.numel() else float('nan'))
    bdry = int(positive.numel() / 4)
    print(positive.numel())
    if bdry < grid_size:
        return None
    order = torch.argsort(counts, -1, True)
    pick = torch.from_numpy(np.random.choice(bdry, grid_size, replace=False)).to(images.device)
    return images[order[:bdry][pick]]


def plot_color_mnist_generator(netG, save_path=None, file_name='plot_generator', num_data=10000):
    """num_data samples of netG: the first 100 as {file_name}_all.jpg, and six of the greenest and six of the reddest quarter as
    {file_name}_green.jpg / {file_name}_red.jpg (plot.py:269-318).  The samples stay on the device; counts, argsort and quantiles
    are torch ops there.  num_data: 10 000 in the reference."""
    print(f'plot_color_mnist_generator file_name: {file_name}')
    grid_size = 6
    netG.eval()
    with torch.no_grad():
        test_imgs = netG.generate_images(num_data, 'cuda').detach().to('cuda')
        show_images_grid(test_imgs, num_images=100, save_path=save_path, file_name=f'{file_name}_all')
        plot_dict = dict()
        for name, channel in (('green', 1), ('red', 0)):
            picked = _positive_quarter(test_imgs, channel, grid_size)
            if picked is not None:
                plot_dict[name] = picked
    for name, imgs in plot_dict.items():
        show_images_grid(imgs, num_images=grid_size, save_path=save_path, file_name=f'{file_name}_{name}')
    netG.train()


def plot_mnist_fmnist_generator(netG, save_path=None, file_name='plot_generator', num_data=10000, batch_size=100):
    """num_data samples of netG in batches of batch_size, the first 100 as {file_name}_all.jpg (plot.py:321-338).  Every batch is
    generated, as in the reference, so the generators end where they end there; only what the picture shows is kept."""
    print(f'plot_color_mnist_generator file_name: {file_name}')
    netG.eval()
    with torch.no_grad():
        shown = []
        for i in range(num_data // batch_size):
            tmp_imgs = netG.generate_images(batch_size, 'cuda').detach()
            if sum(t.shape[0] for t in shown) < 100:
                shown.append(tmp_imgs)
        show_images_grid(torch.cat(shown, 0), num_images=100, save_path=save_path, file_name=f'{file_name}_all')
    netG.train()
