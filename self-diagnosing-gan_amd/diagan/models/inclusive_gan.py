"""Inclusive GAN baseline on the MNIST_DCGAN pair (reference: diagan-pkg/diagan/models/inclusive_gan.py; the Colored-MNIST and
MNIST/FMNIST tables of the paper).  Same class, method and constructor-keyword names.

Every `S = 20 num_data / batch_size` steps the generator draws `latent_factor * num_data` latents and, for each training image,
keeps the latent whose generated image is nearest in the FID Inception pool-3 feature space (:151-213).  Each step logs
    errG = advG + lamb * reconsG + beta * itpG                                                                       (:342)
where reconsG and itpG are feature-space distances between real images and the images of their (noised, interpolated) nearest
latents (:269-338).  Everything stays on the device: the Inception network is diagan.models.inception (HIP, inference only), the
nearest-latent search is diagan.ops.nn_search (one fused GEMM + argmin); there are no NumPy round trips.

**The feature terms carry no gradient.**  The reference computes them under `torch.no_grad()` and through `.cpu().numpy()`
(get_activations, :61-69), and the Inception network here has no backward.  The parameter update is therefore exactly
BaseGenerator's on advG (`adversarial_grads` + `optG.step()`); reconsG and itpG only enter the logged loss.  What the extra
forwards do change are the BatchNorm running statistics: they run in the module's current mode (:292-293,327), as does the
refresh sweep (:162).

Departures from the reference, on purpose:
  * get_activations there runs `len(images) // 50` batches of 50 and leaves the remaining rows of its `np.empty` result
    uninitialised (:47-49); a 64- or 128-image call returns memory garbage in rows 50.. / 100...  Here every row is computed.
  * the nearest-latent search breaks ties between bit-equal distances by the lowest index, whatever the chunking; the
    reference's rule (first index inside a 64-chunk, the LATER chunk between chunks, :189-197) depends on its chunk size.
  * the candidate latents are drawn on the device (one `torch.randn`), not on the host (:156).
  * a one-channel generator (`nc=1`, mnist_fmnist) has its image repeated over the three Inception input channels; the
    reference's Inception network would reject the one-channel tensor.
"""
from copy import deepcopy

import torch

from diagan.models import base as _base
from diagan.models.inception import InceptionV3
from diagan.models.mnist import MNIST_DCGAN_Generator
from diagan.ops.nn_search import NearestSearch, nearest_rows

__all__ = ['get_activations', 'InclusiveMNISTDCGANGenerator']


def get_activations(images, model, batch_size=50, dims=2048, device='cpu', verbose=True):
    """Pool-3 (or `dims`-wide) Inception features of `images` [N, C, H, W] as a float32 DEVICE tensor [N, dims] (reference
    :23-79 returns a float64 NumPy array).  Images go to the network as they are -- the generator's tanh range, the loader's
    range -- and the network's own `normalize_input` maps them by 2 x - 1, as in the reference.  All N rows are computed, in
    batches of `batch_size` with a shorter last one (see the module docstring; the features of an image do not depend on its
    batch).  `device`: where the images are moved to (the HIP engine needs a GPU)."""
    model.eval()
    if not torch.device(device).type == 'cuda':
        raise RuntimeError("get_activations: the HIP engine needs a GPU device (no CPU fallback)")
    n = len(images)
    if n == 0:
        return torch.empty((0, dims), dtype=torch.float32, device=device)
    batch_size = max(1, min(int(batch_size), n))
    out = torch.empty((n, dims), dtype=torch.float32, device=device)
    with torch.no_grad():
        for start in range(0, n, batch_size):
            batch = images[start:start + batch_size].to(device=device, dtype=torch.float32)
            if batch.shape[1] == 1:
                batch = batch.expand(-1, 3, -1, -1)
            out[start:start + batch.shape[0]] = model.features(batch.contiguous(), dims=dims)
            if verbose:
                print("\rINFO: Propagated batch %d/%d" % (start // batch_size + 1, -(-n // batch_size)), end="", flush=True)
    return out


class InclusiveMNISTDCGANGenerator(MNIST_DCGAN_Generator):
    """MNIST_DCGAN_Generator with the Inclusive GAN step (reference :82-369).

    Constructor keywords as in the reference: `num_data` or `dataset` ('cifar10' / 'celeba' sizes, :89-99), `dataloader`
    (batches of (image, target, weight, index)), `loss_type`, `topk`, `nc`.  Keyword-only extras: `inception` -- a ready
    InceptionV3, or a weights object / path for one (None: the file named by DIAGAN_FID_WEIGHTS); `latent_factor` -- candidate
    latents per training image (the reference's 10, :155)."""

    # The step reads a data loader and branches on global_step: it must never be replayed as a captured graph.  launch_bound
    # keeps LogTrainer's automatic capture away; graph_capturable also refuses a forced one (DIAGAN_GRAPH=1).
    launch_bound = False
    graph_capturable = False

    SIGMA = 0.05          # :250
    LAMB = 10             # :251
    BETA = 0.4 * 10       # :252  (0.4 * lamb)
    SWEEP_BATCH = 128     # :154

    def __init__(self, loss_type='ns', *, inception=None, latent_factor=10, **kwargs):
        print(f"Load DCGAN InclusiveGenerator loss_type: {loss_type}")
        MNIST_DCGAN_Generator.__init__(self, loss_type=loss_type, **kwargs)
        self.loss_type = loss_type
        if 'num_data' in kwargs:                                   # :89-99
            self.num_data = kwargs['num_data']
        elif 'dataset' in kwargs:
            if kwargs['dataset'] == 'cifar10':
                self.num_data = 50000
            elif kwargs['dataset'] == 'celeba':
                self.num_data = 162770
            else:
                raise NotImplementedError
        else:
            raise ValueError("InclusiveMNISTDCGANGenerator needs num_data or dataset")
        if 'dataloader' in kwargs:                                 # :101-104
            self.dataloader = kwargs['dataloader']
        else:
            raise ValueError("InclusiveMNISTDCGANGenerator needs dataloader")
        if int(latent_factor) < 1:
            raise ValueError(f"latent_factor must be at least 1, got {latent_factor}")
        self.latent_factor = int(latent_factor)
        self._inception_arg = inception
        self.setting = False
        self.last_terms = None
        self.stack_train_feats = None
        self.nearest_latent = None
        self.nearest_idx = None

    def get_setting(self, train=True):
        """The distance, the feature network and (train) the training features (reference :108-117)."""
        self.pdist = torch.nn.PairwiseDistance(p=2)
        net = self._inception_arg
        if not isinstance(net, InceptionV3):
            net = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[2048]], weights=net)
        # not a registered submodule: the generator's parameters, buffers, checkpoints and flat slabs stay MNIST_DCGAN's
        object.__setattr__(self, 'inception', net.to(self.device))
        if train:
            self.register_train_dataset_feats()
        self.setting = True

    def _features(self, images):
        return get_activations(images, model=self.inception, batch_size=self.SWEEP_BATCH, device=self.device, verbose=False)

    def register_train_dataset_feats(self, path=None):
        """stack_train_feats[i] = the features of the training item with the i-th smallest dataset index (reference :120-148:
        a dict keyed by index, a later visit of the same index replacing the earlier, stacked in key order).  One walk over
        the loader; `path` is unused there too."""
        feats, idxs = [], []
        for data, _, _, idx in iter(self.dataloader):
            feats.append(self._features(data))
            idxs.append(torch.as_tensor(idx).to(self.device, torch.int64).view(-1))
        feats, idxs = torch.cat(feats), torch.cat(idxs)
        keys, inverse = torch.unique(idxs, sorted=True, return_inverse=True)
        last = torch.zeros(keys.numel(), dtype=torch.int64, device=self.device)
        last.scatter_reduce_(0, inverse, torch.arange(idxs.numel(), device=self.device), reduce='amax', include_self=True)
        self.stack_train_feats = feats[last].contiguous()

    def get_latent_dataset_feats(self, path=None, consume=None):
        """Draws the candidate latents (ONE torch.randn on the device) and forwards them in splits of 128 under no_grad, in the
        module's current mode (reference :151-176).  Returns (feats, latent_candidate).  With `consume`, every split's
        features are handed to it as they are produced and feats is None: the latent_factor * num_data x 2048 matrix is
        never held whole."""
        num_latent = self.num_data * self.latent_factor
        latent_candidate = torch.randn((num_latent, self.nz), device=self.device)
        parts = []
        with torch.no_grad():
            for z in torch.split(latent_candidate, self.SWEEP_BATCH):
                data_feats = self._features(self.forward(z).detach())
                if consume is not None:
                    consume(data_feats)
                else:
                    parts.append(data_feats)
        return (torch.cat(parts) if consume is None else None), latent_candidate

    def get_min_latent_idxs(self, latent_feats, batch_size=50):
        """For every row of stack_train_feats the index of the nearest row of latent_feats (reference :178-199; `batch_size`
        was its chunk width and is not needed by the fused search).  Ties: the lowest index."""
        return nearest_rows(self.stack_train_feats, latent_feats.to(self.device, torch.float32))[0]

    def compute_nearest_latent(self, batch_size=64):
        """nearest_latent[i] = the candidate latent whose image is nearest to training item i (reference :210-213)."""
        search = NearestSearch(self.stack_train_feats)
        _, latent_candidate = self.get_latent_dataset_feats(consume=search.update)
        self.nearest_idx = search.result()[0]
        self.nearest_latent = latent_candidate[self.nearest_idx]

    def train_step(self, real_batch, netD, optG, log_data, device=None, global_step=None, scaler=None, noise=None, **kwargs):
        """One G step (reference :215-369).  Draws on the device generator, in order: [the refresh's candidates when
        global_step % S == 0,] z of the adversarial batch (and, in training mode, D's dropout masks) inside
        BaseGenerator.adversarial_grads, noise1, noise2, alpha; the two comparison batches are the first two of a fresh
        iterator over a deepcopy of the loader (:270-273; its shuffle draws from the host generator).  The three extra
        forwards see the parameters BEFORE this step's update, as there (optG.step() is the reference's last act, :344).
        `last_terms` keeps advG, reconsG, itpG of this step as device scalars."""
        if scaler is not None:
            raise NotImplementedError("amp/GradScaler is not part of the fp32 MI355X path")      # reference :346-347
        if _base._world_size() > 1:
            raise NotImplementedError("the Inclusive GAN step is single-GPU (as train_mimicry_inclusive.py is)")
        if not self.setting:
            self.get_setting()
        device = self.device if device is None else device
        batch_size = real_batch[0].shape[0]
        S = int(self.num_data / batch_size * 20)                                                   # :249
        if global_step % S == 0:                                                                   # :254-255
            self.compute_nearest_latent()

        advG = self.adversarial_grads(real_batch, netD, optG, device=device, noise=noise)[0]

        with torch.no_grad():
            copy_dataiter = iter(deepcopy(self.dataloader))                                        # :270-273
            comp_batch1 = next(copy_dataiter)
            comp_batch2 = next(copy_dataiter)
            del copy_dataiter
            comp_idx1 = torch.as_tensor(comp_batch1[3]).to(device, torch.int64)
            comp_idx2 = torch.as_tensor(comp_batch2[3]).to(device, torch.int64)
            comp_feat1 = self.stack_train_feats[comp_idx1]
            comp_feat2 = self.stack_train_feats[comp_idx2]
            nearest_latent1 = self.nearest_latent[comp_idx1]
            nearest_latent2 = self.nearest_latent[comp_idx2]
            noise1 = torch.normal(mean=torch.zeros_like(nearest_latent1), std=self.SIGMA * torch.ones_like(nearest_latent1))
            noise2 = torch.normal(mean=torch.zeros_like(nearest_latent2), std=self.SIGMA * torch.ones_like(nearest_latent2))
            nz1 = nearest_latent1 + noise1
            nz2 = nearest_latent2 + noise2
            gen1_feats = self._features(self.forward(nz1))
            gen2_feats = self._features(self.forward(nz2))
            reconsG = 0.5 * torch.mean(self.pdist(gen1_feats, comp_feat1) + self.pdist(gen2_feats, comp_feat2))   # :317
            alpha = torch.rand(len(nz1), device=device)                                            # :323-327
            alpha_reshape = torch.unsqueeze(alpha, 1)
            itp_z = torch.mul(alpha_reshape, nz1) + torch.mul(1 - alpha_reshape, nz2)
            gen_itp_feats = self._features(self.forward(itp_z))
            itpG = torch.mean(alpha * self.pdist(gen_itp_feats, comp_feat1)
                              + (1 - alpha) * self.pdist(gen_itp_feats, comp_feat2))               # :337-338
            errG = advG + self.LAMB * reconsG + self.BETA * itpG                                   # :342

        optG.step()
        self.last_terms = dict(advG=advG, reconsG=reconsG, itpG=itpG)
        log_data.add_metric('errG', errG, group='loss')
        return log_data
