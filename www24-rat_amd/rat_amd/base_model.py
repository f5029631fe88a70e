"""BaseModel — the training-loop surface the reference's driver calls (run_expid.py:75-102), re-hosted on the HIP
hot path.  Same public methods, kwargs, log lines and checkpoint format as fuxictr/pytorch/models/base_model.py
(cited per method); the arithmetic (loss, regulariser, clipping, Adam) runs in librat_hip.so over flat buffers.
"""
import logging
import os
import re

import numpy as np
import torch
from torch import nn

from .metrics import device_metrics as evaluate_metrics_on_device
from .metrics import is_grouped as is_grouped_metric
from .metrics import evaluate_metrics


def get_device(gpu=-1):
    """torch_utils.py:34-39."""
    if gpu >= 0 and torch.cuda.is_available():
        return torch.device("cuda:%d" % gpu)
    return torch.device("cpu")


def seed_everything(seed=1029):
    """torch_utils.py:26-32."""
    import random
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


def parse_regularizer(reg):
    """get_regularizer (torch_utils.py:65-81) restricted to what the HIP path implements: a float or "l2(x)"."""
    if not reg:
        return 0.0
    if isinstance(reg, (int, float)):
        return float(reg)
    if isinstance(reg, str) and reg.startswith("l2("):
        return float(reg.rstrip(")").split("(")[-1])
    raise NotImplementedError("regularizer=%r: only l2 is implemented on the HIP path" % (reg,))


class Monitor:
    """fuxictr/utils.py:94-104."""

    def __init__(self, kv):
        self.kv_pairs = {kv: 1} if isinstance(kv, str) else kv

    def get_value(self, logs):
        return sum(logs.get(k, 0) * v for k, v in self.kv_pairs.items())


class BaseModel(nn.Module):
    def __init__(self, feature_map, model_id="BaseModel", gpu=-1, monitor="AUC", save_best_only=True,
                 monitor_mode="max", patience=2, every_x_epochs=1, embedding_regularizer=None, net_regularizer=None,
                 reduce_lr_on_plateau=True, embedding_initializer="torch.nn.init.normal_(std=1e-4)",
                 retrieval_augmented=False, retrieval_configs=None, device_metrics=False, group_id=None, **kwargs):
        """device_metrics: evaluate_generator computes its metrics on the device (metrics.device_metrics: 64 bytes come back instead of
        every prediction and label).  group_id: the categorical feature whose id on the target row groups the rows for "GAUC" and the
        ranking names "NDCG(k=K)", "MRR(k=K)", "HitRate(k=K)"."""
        super().__init__()
        self.device = get_device(gpu)
        self._monitor = Monitor(kv=monitor)
        self._monitor_mode = monitor_mode
        self._patience = patience
        self._every_x_epochs = every_x_epochs
        self._save_best_only = save_best_only
        self._embedding_regularizer = embedding_regularizer
        self._net_regularizer = net_regularizer
        self._reduce_lr_on_plateau = reduce_lr_on_plateau
        self._embedding_initializer = embedding_initializer
        self._retrieval_augmented = retrieval_augmented
        if retrieval_augmented:
            assert retrieval_configs is not None, \
                "retrieval-augmented mode requires a dataset with retrieval configurations"
            self._labelwise_retrieval = retrieval_configs["label_wise"]
        self._feature_map = feature_map
        self.model_id = model_id
        self.model_dir = os.path.join(kwargs["model_root"], feature_map.dataset_id)
        self.checkpoint = os.path.abspath(os.path.join(self.model_dir, self.model_id + ".model"))
        self._validation_metrics = kwargs["metrics"]
        self._device_metrics = bool(device_metrics)
        self._group_id, self._group_col = group_id, None
        if group_id is not None:
            spec = feature_map.feature_specs.get(group_id)
            if spec is None:
                raise ValueError("group_id=%r is not a feature of this dataset" % (group_id,))
            if spec["type"] != "categorical":
                raise ValueError("group_id=%r is a %s field: GAUC groups by one id per row, so it takes a plain categorical field"
                                 % (group_id, spec["type"]))
            self._group_col = int(spec["index"])
        for metric in (self._validation_metrics or []):
            if is_grouped_metric(metric) and group_id is None:
                raise ValueError('metrics holds "%s" but no group_id names the feature to group by' % metric)
        self._refuse_new_eval_options_under_dp()
        self._verbose = kwargs["verbose"]
        self._max_gradient_norm = 10.0

    # ---- compile / loss ------------------------------------------------------------------------------
    def compile(self, optimizer, loss, lr):
        """base_model.py:70-72 (torch_utils.get_optimizer / get_loss_fn): "adam" in any case, or a torch.optim class name — Adam, SGD,
        Adagrad, RMSprop have kernels (clip + update over the flat buffers); the loss / task pairs the head kernels fuse: see below."""
        from .optim import KINDS, FusedClipAdam
        if not isinstance(optimizer, str):
            raise NotImplementedError("optimizer=%r: pass a name" % (optimizer,))
        if optimizer.lower() == "adam":
            optimizer = "Adam"
        if optimizer not in KINDS:
            raise NotImplementedError("optimizer=%r is not supported on the HIP path (have %s)" % (optimizer, ", ".join(KINDS)))
        # the head kernels (rat_logit_fwd / rat_logit_bwd) fuse output activation and loss: Sigmoid + binary cross-entropy for
        # task = "binary_classification" (every shipped config), no activation + F.mse_loss for task = "regression"
        # (base_model.py:286-292, torch_utils.get_loss_fn: torch_utils.py:51-63)
        task = getattr(self, "_task", "binary_classification")
        if loss in ("bce", "binary_crossentropy", "binary_cross_entropy") and task == "binary_classification":
            self.loss_fn, self._head = "binary_cross_entropy", 0
        elif loss in ("mse_loss", "mse") and task == "regression":
            self.loss_fn, self._head = "mse_loss", 1
        else:
            raise NotImplementedError("task=%r with loss=%r: the HIP head implements binary_classification + binary cross-entropy and "
                                      "regression + mse_loss" % (task, loss))
        self.optimizer = FusedClipAdam(self, lr=lr, kind=optimizer)

    def add_loss(self, inputs, reduction="mean"):
        """base_model.py:74-77."""
        assert reduction == "mean"
        return self._loss_terms(inputs, with_reg=False)[1]

    def add_regularization(self):
        """base_model.py:79-94: (lambda/2)*||W||^2 over the "embedding_layer" tensors (and net_regularizer over the rest)."""
        return self._regularization_value()

    def get_total_loss(self, inputs):
        """base_model.py:97-99: BCE + regulariser, one autograd node whose backward is the HIP backward pass."""
        _, loss, reg = self._loss_terms(inputs, with_reg=True)
        total = loss + reg
        world = self._world_size()
        return total / world if world > 1 else total

    # ---- init ----------------------------------------------------------------------------------------
    def reset_parameters(self):
        """base_model.py:101-123: N(0, std) on every nn.Embedding that lives in an nn.ModuleDict (all rows but
        the last when a padding row exists), xavier_normal_ + zero bias on every nn.Linear.  Visiting order is
        nn.Module.apply's, so the RNG stream matches the reference's for an identical module tree."""
        init = self._embedding_initializer
        std = None
        if init is not None:
            m = re.fullmatch(r"torch\.nn\.init\.normal_\(std=([0-9.eE+-]+)\)", init.replace(" ", ""))
            if m is None:
                raise NotImplementedError("embedding_initializer={} is not supported.".format(init))
            std = float(m.group(1))

        def visit(mod):
            if type(mod) == nn.ModuleDict:
                for _, v in mod.items():
                    if type(v) == nn.Embedding and std is not None:
                        target = v.weight[0:-1, :] if v.padding_idx is not None else v.weight
                        torch.nn.init.normal_(target, std=std)
            if type(mod) == nn.Linear:
                nn.init.xavier_normal_(mod.weight)
                if mod.bias is not None:
                    mod.bias.data.fill_(0)
        with torch.no_grad():
            self.apply(visit)

    def inputs_to_device(self, inputs):
        """base_model.py:125-139 — kept for API compatibility; the HIP path uses _prepare_batch instead."""
        if self._retrieval_augmented:
            X, y, retrieved_values, retrieved_lens = inputs
            self.batch_size = y.size(0)
            return (X.to(self.device), y.float().unsqueeze(-1).to(self.device), retrieved_values.to(self.device),
                    retrieved_lens.int().to(self.device))
        X, y = inputs
        self.batch_size = y.size(0)
        return X.to(self.device), y.float().unsqueeze(-1).to(self.device)

    def model_to_device(self):
        self.to(device=self.device)
        self._after_device_move()

    # ---- fit -----------------------------------------------------------------------------------------
    # The training-loop contract of the reference (base_model.py:144-211) is kept — same public methods, same attributes that
    # tooling reads (_best_metric, _stopping_steps, _stop_training, _total_batches), same log lines (the
    # experiment scripts parse them) — but organised around one small state record and two helpers: `_validation_due` decides
    # WHEN to validate, `_judge` turns a monitored value into (improved?, stop?).  Under data parallelism every rank takes
    # the decision from rank 0's value and only rank 0 writes the checkpoint.
    @staticmethod
    def freeze_host_heap():
        """Keep the interpreter's garbage collector out of the training loop's way: after `import torch` the process holds
        ~10^6 long-lived container objects, and every full (generation-2) collection — one per ~10 steps at this loop's
        allocation rate — walks all of them: a 110-150 ms host stall measured on the MI355X box, i.e. five whole training
        steps at the north-star shape.  gc.freeze() moves everything alive NOW into the permanent generation; collection of
        the loop's own garbage stays enabled."""
        import gc
        gc.collect()
        gc.freeze()

    def _validation_due(self, batch_index):
        """validate every `every_x_epochs` epochs' worth of batches and at the end of every epoch (base_model.py:146)"""
        done = batch_index + 1
        return done % self._every_x_batches == 0 or done % self._batches_per_epoch == 0

    def on_batch_end(self, batch, logs={}):
        """base_model.py:144-151."""
        self._total_batches += 1
        if not self._validation_due(batch):
            return
        epoch = round(self._total_batches / float(self._batches_per_epoch), 2)
        self.checkpoint_and_earlystop(epoch, self.evaluate_generator(self.valid_gen))
        self.train()
        logging.info("--- {}/{} batches finished ---".format(batch + 1, self._batches_per_epoch))

    def lr_decay(self, factor=0.1, min_lr=1e-6):
        """base_model.py:153-158: every param group's lr <- max(lr * factor, min_lr); returns the last one."""
        lrs = [max(group["lr"] * factor, min_lr) for group in self.optimizer.param_groups]
        for group, lr in zip(self.optimizer.param_groups, lrs):
            group["lr"] = lr
        return lrs[-1] if lrs else None

    def _agreed_value(self, value):
        """Data parallelism: all ranks act on rank 0's monitored value (validation shards may differ per rank; a rank that
        stopped or decayed alone would dead-lock the next all-reduce)."""
        if self._dp():
            import torch.distributed as dist
            box = torch.tensor([value], dtype=torch.float64, device=self.device if self.device.type == "cuda" else "cpu")
            dist.broadcast(box, src=0)
            value = float(box[0])
        return value

    def _judge(self, value, min_delta):
        """-> True when `value` improves on the best so far by more than min_delta in the monitored direction"""
        if self._monitor_mode == "min":
            return value <= self._best_metric - min_delta
        return value >= self._best_metric + min_delta

    def _save_checkpoint(self):
        if self._rank() == 0:
            self.save_weights(self.checkpoint)
        if self._dp():
            import torch.distributed as dist
            dist.barrier()

    def checkpoint_and_earlystop(self, epoch, logs, min_delta=1e-6):
        """base_model.py:160-179."""
        value = self._agreed_value(self._monitor.get_value(logs))
        if self._judge(value, min_delta):
            self._stopping_steps, self._best_metric = 0, value
            if self._save_best_only:
                logging.info("Save best model: monitor({}): {:.6f}".format(self._monitor_mode, value))
                self._save_checkpoint()
        else:
            self._stopping_steps += 1
            logging.info("Monitor({}) STOP: {:.6f} !".format(self._monitor_mode, value))
            if self._reduce_lr_on_plateau:
                logging.info("Reduce learning rate on plateau: {:.6f}".format(self.lr_decay()))
        if not self._save_best_only:
            self._save_checkpoint()
        if self._stopping_steps * self._every_x_epochs >= self._patience:
            self._stop_training = True
            logging.info("Early stopping at epoch={:g}".format(epoch))

    def fit_generator(self, data_generator, epochs=1, validation_data=None, verbose=0, max_gradient_norm=10., **kwargs):
        """base_model.py:181-211."""
        self.freeze_host_heap()
        self.valid_gen, self._verbose, self._max_gradient_norm = validation_data, verbose, max_gradient_norm
        self._batches_per_epoch = len(data_generator)
        self._every_x_batches = int(np.ceil(self._every_x_epochs * self._batches_per_epoch))
        self._best_metric = {"min": np.inf}.get(self._monitor_mode, -np.inf)
        self._stopping_steps = self._total_batches = 0
        self._stop_training = False
        logging.info("Start training: {} batches/epoch".format(self._batches_per_epoch))
        logging.info("************ Epoch=1 start ************")
        epoch = 0
        while epoch < epochs and not self._stop_training:
            logging.info("Train loss: {:.6f}".format(self.train_one_epoch(data_generator, epoch)))
            epoch += 1
            if not self._stop_training:
                logging.info("************ Epoch={} end ************".format(epoch))
        logging.info("Training finished.")

    def train_step(self, batch_data):
        """One iteration of base_model.py:220-226: zero_grad -> loss -> backward -> clip(10.) -> Adam.
        Returns the (device) loss tensor; no host synchronisation.  The concrete model may run the whole iteration as one fused
        pass over its flat buffers (RAT_m2._fused_train_step: no autograd node, regulariser folded into a two-sweep optimizer,
        optionally replayed as a captured hipGraph); `train_step_reference_order` is the literal sequence."""
        fused = getattr(self, "_fused_train_step", None)
        if fused is not None and self.fused_step:
            return fused(batch_data)
        return self.train_step_reference_order(batch_data)

    fused_step = True          # set False to make train_step run the literal zero_grad / backward / clip / step sequence

    def train_step_reference_order(self, batch_data):
        self.optimizer.zero_grad()
        loss = self.get_total_loss(batch_data)
        loss.backward()
        self._exchange_gradients()
        self.optimizer.clip_and_step(self._max_gradient_norm)
        return loss.detach()

    def train_one_epoch(self, data_generator, epoch):
        self.train()
        running = torch.zeros((), device=self.device)
        for batch_index, batch_data in enumerate(data_generator):
            running += self.train_step(batch_data) * self._world_size()
            if self.valid_gen is not None:
                self.on_batch_end(batch_index)
            else:
                self._total_batches += 1
            if self._stop_training:
                break
        epoch_loss = float(running.item()) / self._batches_per_epoch
        self.check_id_errors()
        return epoch_loss

    # ---- eval ----------------------------------------------------------------------------------------
    shard_evaluation = True    # data parallelism: every rank evaluates 1/world of each batch, the predictions are all-gathered

    def evaluate_generator(self, data_generator):
        """base_model.py:232-247.  Under data parallelism (and a batch source that can shard: rat_amd.data) each rank runs the forward
        on its slice of every batch — nothing is dropped — and all ranks compute the metrics from the all-gathered predictions, so they
        agree on early stopping / lr decay by construction."""
        if self._device_metrics or self._group_col is not None:
            return self._evaluate_generator_options(data_generator)
        self.eval()
        preds, trues = [], []
        world = self._world_size()
        sharded = bool(self.shard_evaluation and self._dp() and world > 1 and getattr(data_generator, "shard", None) == (0, 1))
        if sharded:
            data_generator.shard, data_generator.keep_all = (self._rank(), world), True
        try:
            with torch.no_grad():
                for batch_data in data_generator:
                    out = self.forward(batch_data)
                    preds.append(out["y_pred"])
                    trues.append(out["y_true"])
        finally:
            if sharded:
                data_generator.shard, data_generator.keep_all = (0, 1), False
        empty = torch.zeros((0, 1), dtype=torch.float32, device=self.device)
        y_pred, y_true = torch.cat(preds or [empty]).reshape(-1), torch.cat(trues or [empty]).reshape(-1)
        if sharded:
            y_pred, y_true = self._gather_ragged(y_pred, y_true)
        y_pred = y_pred.double().cpu().numpy().reshape(-1)
        y_true = y_true.double().cpu().numpy().reshape(-1)
        self.check_id_errors()
        return self.evaluate_metrics(y_true, y_pred, self._validation_metrics)

    def _gather_ragged(self, *vectors):
        """all-gather of equally long float vectors whose length differs from rank to rank -> the concatenation over ranks, in rank order"""
        import torch.distributed as dist
        world = self._world_size()
        staged = dist.get_backend() == "gloo"
        dev = torch.device("cpu") if staged else self.device
        n = torch.tensor([vectors[0].numel()], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(counts, n)
        counts = [int(c[0]) for c in counts]
        cap = max(max(counts), 1)
        mine = torch.zeros((len(vectors), cap), dtype=torch.float32, device=dev)
        for i, v in enumerate(vectors):
            mine[i, :v.numel()] = v.to(dev, torch.float32)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
        return tuple(torch.cat([parts[r][i, :counts[r]] for r in range(world)]) for i in range(len(vectors)))

    def evaluate_metrics(self, y_true, y_pred, metrics, group_index=None):
        return evaluate_metrics(y_true, y_pred, metrics, group_index=group_index)

    def _refuse_new_eval_options_under_dp(self):
        if (self._device_metrics or self._group_id is not None) and self._dp():
            raise ValueError("device_metrics / group_id are not available under data parallelism: the ranks evaluate shards of every "
                             "batch and all-gather predictions and labels only — neither the metric chain nor the group ids are "
                             "exchanged.  Evaluate on one device, or drop the two options")

    def _evaluate_generator_options(self, data_generator):
        """evaluate_generator with device_metrics and / or group_id: predictions, labels and (for "GAUC" and the ranking names) the target rows' ids of the
        group column stay on the device.  With device_metrics the metric chain runs there and 64 bytes come back; without, the three
        vectors are copied once and metrics.evaluate_metrics runs on the host as before."""
        self._refuse_new_eval_options_under_dp()
        self.eval()
        metrics = self._validation_metrics
        col = self._group_col if any(is_grouped_metric(m) for m in metrics) else None
        preds, trues, groups = [], [], []
        with torch.no_grad():
            for batch_data in data_generator:
                out = self.forward(batch_data)
                preds.append(out["y_pred"].reshape(-1))
                trues.append(out["y_true"].reshape(-1))
                if col is not None:
                    ids = batch_data.idx if hasattr(batch_data, "idx") else batch_data[0]      # DeviceBatch or the 4-tuple
                    groups.append(ids[:, 0, col].to(self.device, torch.int32).clone())
        empty = torch.zeros((0,), dtype=torch.float32, device=self.device)
        y_pred, y_true = torch.cat(preds or [empty]), torch.cat(trues or [empty])
        group = torch.cat(groups or [empty.to(torch.int32)]) if col is not None else None
        self.check_id_errors()
        if self._device_metrics:
            return evaluate_metrics_on_device(y_true, y_pred, metrics, group_index=group, lib=getattr(self, "_lib", None))
        return self.evaluate_metrics(y_true.double().cpu().numpy(), y_pred.double().cpu().numpy(), metrics,
                                     group_index=None if group is None else group.cpu().numpy())

    def predict_generator(self, data_generator):
        """base_model.py:252-273."""
        self.eval()
        preds = []
        with torch.no_grad():
            for batch_data in data_generator:
                ids = batch_data.idx if hasattr(batch_data, "idx") else batch_data[0]      # DeviceBatch or the 4-tuple
                assert ids.ndim == 3, "retrieval augmented mode requires input_shape like [Bx(1+K)xF]"
                preds.append(self.forward(batch_data)["y_pred"])
        out = torch.cat(preds).double().cpu().numpy().reshape(-1)
        self.check_id_errors()
        return out

    def save_weights(self, checkpoint):
        os.makedirs(os.path.dirname(os.path.abspath(checkpoint)), exist_ok=True)
        torch.save(self.state_dict(), checkpoint)

    def load_weights(self, checkpoint):
        state = torch.load(checkpoint, map_location="cpu")
        self.load_state_dict(state)          # copies in place: the flat parameter buffer stays intact

    def get_output_activation(self, task="binary_classification"):
        """base_model.py:286-292"""
        self._task = task
        if task == "binary_classification":
            return nn.Sigmoid()
        if task == "regression":
            return None
        raise NotImplementedError("task={} is not supported.".format(task))

    def count_parameters(self, count_embedding=True):
        """base_model.py:294-301."""
        total = 0
        for name, p in self.named_parameters():
            if not count_embedding and "embedding" in name:
                continue
            if p.requires_grad:
                total += p.numel()
        logging.info("Total number of parameters: {}.".format(total))
        return total

    # ---- hooks the concrete model fills in -----------------------------------------------------------
    def _after_device_move(self):
        pass

    def _world_size(self):
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    # A process group of ONE rank normally trains like a single process (no collective is issued).  dp_single_rank = True sends it
    # through the data-parallel code path anyway — every all-reduce / all-gather / barrier of a step, on one rank: the only way a
    # 1-GPU box can put the RCCL calls of the N > 1 path on real hardware (tests/test_gpu_rccl.py).
    dp_single_rank = False

    def _dp(self):
        """the data-parallel code path is active"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return False
        return dist.get_world_size() > 1 or self.dp_single_rank

    def _rank(self):
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def _exchange_gradients(self):
        pass

    def check_id_errors(self):
        pass
