"""main.py-equivalent training harness for APPNP on the HIP propagation path.

Reproduces the call pattern of /root/reference/main.py:63-175:

* seeds (helpers.py:13-17)
* L1 attribute normalisation (preprocessing.py:54-64)
* known/unknown + train/stopping/validation splits with a fresh uint32 seed per run
  (preprocessing.py:9-52, main.py:33-35, 84-98)
* Adam(lr 0.01) on cross-entropy + reg_lambda/2 * ||W1||^2 (main.py:109-127)
* three forwards per epoch (main.py:121, 138, 145)
* SimpleEarlyStopping with patience 100 (helpers.py:19-55)

The model is ``ppnp_amd.APPNP`` (the dense ``ppnp_amd.PPNP`` with ``--model ppnp``; with
``--model gprgnn`` ``ppnp_amd.GPRGNN``, whose series coefficients are trained with the weights and
are not part of the L2 term), so the
propagation of every forward and backward runs on the fused HIP kernels.  The splitting,
seeding and early stopping are host bookkeeping, restated so that the harness runs without
the reference; tests/test_train.py pins them to the reference's own outputs.

    python -m ppnp_amd.train --dataset cora_ml --n-runs 5      # data: tests/golden/*.npz

With ``--batch-size B --ppr-topk k`` (``--model appnp``) it follows the reference's second entry
point, batch-main.py:104-169, instead: minibatches of top-k-sparsified PPR rows, on the sparse
matrix of ``APPNP.sparse_ppr`` (no N x N matrix; ppnp_amd/ppr.py).  ``--ppr-eps 1e-4`` builds
those rows by forward push, whose work per source does not grow with N; ``--ppr-select lists``
also selects them straight from the push's lists, with no dense block of columns.
``--batch-slice device`` cuts each minibatch out of that matrix with the HIP kernels of
``ops.csr_batch`` (one 24-byte read-back per batch, the transpose for the backward included)
instead of torch operations; the numbers are the same bits.  With it ``--sparse-x`` keeps the
attribute matrix a CSR on the GPU in minibatch training too: ``X[sel]`` becomes ``X.rows(sel)``
and the stopping and validation rows of the PPR matrix ``P.rows(idx, slicer="device")``
(``ops.csr_rows``, one 16-byte read-back each, the transpose included).
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- helpers.py:13-17 ---------------------------------------------------------------------
def set_seeds(seed):
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    torch.manual_seed(seed + 3)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed + 4)


def gen_seeds():
    """main.py:33-35."""
    max_uint32 = np.iinfo(np.uint32).max
    return np.random.randint(max_uint32 + 1, size=1, dtype=np.uint32)


# -- preprocessing.py:9-64 ----------------------------------------------------------------
def exclude_idx(idx, idx_exclude_list):
    idx_exclude = np.concatenate(idx_exclude_list)
    return np.asarray(idx)[~np.isin(idx, idx_exclude)]


def known_unknown_split(idx, nknown=1500, seed=4143496719):
    rnd_state = np.random.RandomState(seed)
    known_idx = rnd_state.choice(idx, nknown, replace=False)
    return known_idx, exclude_idx(idx, [known_idx])


def train_stopping_split(idx, labels, ntrain_per_class=20, nstopping=500, seed=2413340114):
    rnd_state = np.random.RandomState(seed)
    train_idx_split = []
    for i in range(max(labels) + 1):
        train_idx_split.append(rnd_state.choice(idx[labels == i], ntrain_per_class,
                                                replace=False))
    train_idx = np.concatenate(train_idx_split)
    stopping_idx = rnd_state.choice(exclude_idx(idx, [train_idx]), nstopping, replace=False)
    return train_idx, stopping_idx


def gen_splits(labels, idx_split_args, test=False):
    all_idx = np.arange(len(labels))
    known_idx, unknown_idx = known_unknown_split(all_idx, idx_split_args["nknown"])
    stopping_split_args = copy.copy(idx_split_args)
    del stopping_split_args["nknown"]
    train_idx, stopping_idx = train_stopping_split(known_idx, labels[known_idx],
                                                   **stopping_split_args)
    if test:
        val_idx = unknown_idx
    else:
        val_idx = exclude_idx(known_idx, [train_idx, stopping_idx])
    return train_idx, stopping_idx, val_idx


def normalize_attributes(attr_matrix):
    epsilon = 1e-12
    if sp.issparse(attr_matrix):
        attr_norms = np.asarray(abs(attr_matrix).sum(axis=1)).ravel()
        attr_invnorms = 1 / np.maximum(attr_norms, epsilon)
        return sp.csr_matrix(attr_matrix.multiply(attr_invnorms[:, np.newaxis]))
    attr_norms = np.linalg.norm(attr_matrix, ord=1, axis=1)
    attr_invnorms = 1 / np.maximum(attr_norms, epsilon)
    return attr_matrix * attr_invnorms[:, np.newaxis]


# -- helpers.py:19-55 ---------------------------------------------------------------------
class SimpleEarlyStopping:
    def __init__(self, model, patience=100, store_weights=False):
        self.model = model
        self.patience = patience
        self.max_patience = patience
        self.store_weights = store_weights
        self.record = (None,)  # reference quirk: `self.record = None,` (helpers.py:26)
        self.best_acc = -np.inf
        self.best_nloss = -np.inf
        self.best_epoch = -1
        self.best_epoch_score = (-np.inf, -np.inf)

    def should_stop(self, acc, loss, epoch, record=None):
        nloss = -1 * loss
        if (acc < self.best_acc) and (nloss < self.best_nloss):
            self.patience -= 1
            return self.patience == 0
        self.patience = self.max_patience
        self.best_acc = max(acc, self.best_acc)
        self.best_nloss = max(nloss, self.best_nloss)
        if (acc, nloss) > self.best_epoch_score:
            self.best_epoch = epoch
            self.best_epoch_score = (acc, nloss)
            if self.store_weights:
                self.best_state = {k: v.cpu() for k, v in self.model.state_dict().items()}
            if record:
                self.record = record
        return False


# -- data -----------------------------------------------------------------------------------
def load_dataset(name):
    """Standardized LCC adjacency, attributes and labels from tests/golden/<name>.npz (the
    reference's own SparseGraph.standardize output, see tests/golden/make_golden.py)."""
    path = os.path.join(ROOT, "tests", "golden", name)
    d = dict(np.load(path + ".npz", allow_pickle=False))
    if os.path.exists(path + "_attr.npz"):  # a dataset kept in parts: the attribute matrix
        d.update(np.load(path + "_attr.npz", allow_pickle=False))
    n = int(d["n"])
    adj = sp.csr_matrix((d["adj_data"], d["adj_indices"], d["adj_indptr"]), shape=(n, n))
    attr = sp.csr_matrix((d["attr_data"], d["attr_indices"], d["attr_indptr"]),
                         shape=tuple(d["attr_shape"]))
    return adj, attr, np.asarray(d["labels"])


# -- main.py:71-165 -------------------------------------------------------------------------
def run_once(adj, attr, labels, args, device, stats=None):
    from .model import APPNP, GPRGNN, PPNP

    idx_split_args = {"ntrain_per_class": args.ntrain_per_class, "nstopping": args.nstopping,
                      "nknown": args.nknown, "seed": gen_seeds()}
    X = normalize_attributes(attr)
    if args.sparse_x:  # keep X sparse on the GPU (main.py:91 densifies it)
        from .sparse import SparseFeatures

        X = SparseFeatures.from_scipy(X, device=device)
    else:
        X = torch.FloatTensor(np.asarray(X.todense())).to(device)
    y = torch.LongTensor(labels)
    idx_train, idx_stop, idx_valid = gen_splits(labels, idx_split_args, test=args.test)
    idx_train, idx_stop, idx_valid = map(torch.LongTensor, (idx_train, idx_stop, idx_valid))
    y_train, y_stop, y_valid = y[idx_train], y[idx_stop], y[idx_valid]
    idx_train, idx_stop, idx_valid = (t.to(device) for t in (idx_train, idx_stop, idx_valid))
    y_train, y_stop, y_valid = (t.to(device) for t in (y_train, y_stop, y_valid))

    torch.manual_seed(int(gen_seeds()[0]))
    n_classes = int(y.max()) + 1
    if args.model == "ppnp":
        ppr = torch.FloatTensor(_dense_ppr(adj, args.alpha))
        model = PPNP(n_features=X.shape[1], n_classes=n_classes, ppr=ppr).to(device)
    elif args.model == "gprgnn":
        model = GPRGNN(n_features=X.shape[1], n_classes=n_classes, adj=adj, K=args.K,
                       alpha=args.alpha, init=args.coef_init, heat_t=args.heat_t,
                       learn_coef=not args.fixed_coef).to(device)
    else:
        model = APPNP(n_features=X.shape[1], n_classes=n_classes, adj=adj, alpha=args.alpha,
                      K=args.K, edge_drop=args.edge_drop,
                      exact=getattr(args, "exact", False),
                      tol=getattr(args, "tol", 1e-6)).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    early_stopping = SimpleEarlyStopping(model)
    if getattr(args, "batch_size", None):
        return _run_batches(model, opt, early_stopping, X, (idx_train, idx_stop, idx_valid),
                            (y_train, y_stop, y_valid), args, stats)
    t = time.time()
    for epoch in range(args.max_epochs):
        model.train()
        logits = model(X, idx_train)
        train_loss = F.cross_entropy(logits, y_train)
        train_loss = train_loss + args.reg_lambda / 2 * model.get_norm()
        opt.zero_grad()
        train_loss.backward()
        opt.step()
        train_acc = (logits.argmax(dim=-1) == y_train).float().mean()

        model.eval()
        with torch.no_grad():
            logits = model(X, idx_stop)
            stop_loss = F.cross_entropy(logits, y_stop)
            stop_loss = stop_loss + args.reg_lambda / 2 * model.get_norm()
            stop_acc = (logits.argmax(dim=-1) == y_stop).float().mean()
            valid_acc = (model(X, idx_valid).argmax(dim=-1) == y_valid).float().mean()
        record = {"epoch": int(epoch), "elapsed": float(time.time() - t),
                  "train_acc": float(train_acc), "stop_acc": float(stop_acc),
                  "valid_acc": float(valid_acc)}
        if args.verbose:
            print(json.dumps(record), file=sys.stderr)
        if early_stopping.should_stop(acc=float(stop_acc), loss=float(stop_loss), epoch=epoch,
                                      record=record):
            break
    if stats is not None and args.model == "gprgnn":
        stats["coef"] = [float(c) for c in model.coef.detach().cpu()]  # gamma when training ended
    return early_stopping.record


def _run_batches(model, opt, early_stopping, X, idx, y, args, stats=None):
    """batch-main.py:104-169: a shuffled loader over idx_train; per batch the sparsified PPR
    rows of the batch, the union ``sel`` of their columns, ``X[sel]`` and
    ``model(X_batch, ppr=ppr_sub)``; stopping and validation through the sparsified rows too,
    as the reference evaluates on its sparsified buffer.  The records carry the reference's
    keys; the one-time build of the sparse matrix goes to ``stats["ppr_build"]`` (seconds)."""
    from torch.utils.data import DataLoader, TensorDataset

    idx_train, idx_stop, idx_valid = idx
    y_train, y_stop, y_valid = y
    loader = DataLoader(TensorDataset(idx_train.cpu(), y_train.cpu()),
                        batch_size=args.batch_size, shuffle=True, num_workers=0)
    t0 = time.time()
    eps = getattr(args, "ppr_eps", None)
    info = []
    P = model.sparse_ppr(args.ppr_topk, tol=args.tol if args.exact and eps is None else None,
                         eps=eps, info=info, select=getattr(args, "ppr_select", "block"))
    if info:  # forward push: every column must have ended with an empty frontier (one read-back)
        left = torch.cat([l for _, l in info])
        if bool((left != 0).any()):
            raise RuntimeError(f"--ppr-eps {eps}: {int((left != 0).sum())} PPR columns did not "
                               "finish their forward push (max_rounds reached)")
    torch.cuda.synchronize()
    if stats is not None:
        stats["ppr_build"] = time.time() - t0
    sparse_x = not torch.is_tensor(X)  # a SparseFeatures: parse_args allows it with 'device' only
    rows_slicer = "device" if sparse_x else "torch"
    P_stop, P_valid = P.rows(idx_stop, slicer=rows_slicer), P.rows(idx_valid, slicer=rows_slicer)
    t = time.time()
    for epoch in range(args.max_epochs):
        model.train()
        for idx_batch, y_batch in loader:
            ppr_sub, sel = P.batch(idx_batch.to(X.device),
                                   slicer=getattr(args, "batch_slice", "torch"))
            logits = model(X.rows(sel) if sparse_x else X[sel], idx=None, ppr=ppr_sub)
            loss = F.cross_entropy(logits, y_batch.to(X.device))
            loss = loss + args.reg_lambda / 2 * model.get_norm()
            opt.zero_grad()
            loss.backward()
            opt.step()

        model.eval()
        with torch.no_grad():
            logits = model(X, ppr=P_stop)
            stop_loss = F.cross_entropy(logits, y_stop)
            stop_loss = stop_loss + args.reg_lambda / 2 * model.get_norm()
            stop_acc = (logits.argmax(dim=-1) == y_stop).float().mean()
            valid_acc = (model(X, ppr=P_valid).argmax(dim=-1) == y_valid).float().mean()
        record = {"epoch": int(epoch), "elapsed": float(time.time() - t),
                  "stop_acc": float(stop_acc), "valid_acc": float(valid_acc)}
        if args.verbose:
            print(json.dumps(record), file=sys.stderr)
        if early_stopping.should_stop(acc=float(stop_acc), loss=float(stop_loss), epoch=epoch,
                                      record=record):
            break
    return early_stopping.record


def _dense_ppr(adj, alpha):
    """Dense alpha (I - (1-alpha) A_hat)^-1 for --model ppnp (helpers.py:68-71), with A_hat
    from the device build (bit-identical to calc_A_hat in fp32)."""
    from .graph import Graph

    G = Graph.from_scipy(adj, device="cuda")
    rp, col, val, _ = G.csr()
    n = adj.shape[0]
    A = torch.sparse_csr_tensor(rp.long(), col.long(), val.double(), size=(n, n)).to_dense()
    inner = torch.eye(n, dtype=torch.float64, device=A.device) - (1 - alpha) * A
    return (alpha * torch.linalg.inv(inner)).float().cpu()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataset", default="cora_ml")
    p.add_argument("--n-runs", type=int, default=5)
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--ntrain-per-class", type=int, default=20)
    p.add_argument("--nstopping", type=int, default=500)
    p.add_argument("--nknown", type=int, default=1500)
    p.add_argument("--max-epochs", type=int, default=10_000)
    p.add_argument("--reg-lambda", type=float, default=5e-3)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--alpha", type=float, default=0.1)
    p.add_argument("--K", type=int, default=10)
    p.add_argument("--edge-drop", type=float, default=0.0)
    p.add_argument("--exact", action="store_true",
                   help="--model appnp: propagate with the exact PPNP solver (K is ignored)")
    p.add_argument("--tol", type=float, default=1e-6,
                   help="relative tolerance of --exact")
    p.add_argument("--model", default="appnp", choices=["appnp", "ppnp", "gprgnn"])
    p.add_argument("--coef-init", default="ppr", choices=["ppr", "heat"],
                   help="--model gprgnn: the coefficients gamma_k start as the APPNP series of "
                        "--K and --alpha, or as heat-kernel diffusion e^-t t^k / k! (--heat-t)")
    p.add_argument("--heat-t", type=float, default=1.0, help="t of --coef-init heat")
    p.add_argument("--fixed-coef", action="store_true",
                   help="--model gprgnn: keep gamma fixed (a buffer) instead of training it")
    p.add_argument("--sparse-x", action="store_true",
                   help="keep the attribute matrix as a CSR on the GPU (sparse encoder input)")
    p.add_argument("--batch-size", type=int, default=None,
                   help="--model appnp: minibatch training on sparsified PPR rows "
                        "(batch-main.py); needs --ppr-topk")
    p.add_argument("--ppr-topk", type=int, default=None,
                   help="entries kept per column of the PPR matrix (batch-main.py:115-116)")
    p.add_argument("--ppr-eps", type=float, default=None,
                   help="build the sparsified PPR rows by forward push to this threshold "
                        "(ops.push_columns) instead of the series / the solver; needs "
                        "--batch-size")
    p.add_argument("--ppr-select", default=None, choices=["block", "lists"],
                   help="with --ppr-eps: 'lists' selects each source's top k straight from the "
                        "nodes its push took (ops.push_topk, one call for all sources), 'block' "
                        "(the default) from dense N x 128 blocks of columns")
    p.add_argument("--batch-slice", default=None, choices=["torch", "device"],
                   help="with --batch-size: how a minibatch's rows and columns are cut out of "
                        "the sparse PPR matrix: 'torch' (the default) with torch operations, "
                        "'device' with the HIP kernels of ops.csr_batch, which also emit the "
                        "transpose the backward needs (the same bits either way)")
    p.add_argument("--test", action="store_true")
    p.add_argument("--verbose", action="store_true")
    args = p.parse_args(argv)
    if args.model == "gprgnn" and (args.edge_drop > 0 or args.exact):
        p.error("--model gprgnn takes neither --edge-drop nor --exact")
    if args.batch_size is not None:
        if args.batch_size < 1 or not args.ppr_topk or args.ppr_topk < 1:
            p.error("--batch-size needs a positive value and a positive --ppr-topk")
        if args.model != "appnp":
            p.error("--batch-size needs --model appnp")
        if args.sparse_x and args.batch_slice != "device":
            p.error("--batch-size cannot be combined with --sparse-x: a minibatch takes the "
                    "rows X[sel], which needs a dense X (or --batch-slice device, which takes "
                    "them from the sparse X with the HIP kernels of ops.csr_rows)")
        if args.ppr_eps is not None and not 0.0 < args.ppr_eps < 1.0:
            p.error("--ppr-eps must lie in (0, 1)")
    elif args.ppr_topk is not None:
        p.error("--ppr-topk needs --batch-size")
    elif args.ppr_eps is not None:
        p.error("--ppr-eps needs --batch-size and --ppr-topk")
    if args.ppr_select is not None and args.ppr_eps is None:
        p.error("--ppr-select needs --ppr-eps")
    if args.ppr_select is None:
        args.ppr_select = "block"
    if args.batch_slice is not None and args.batch_size is None:
        p.error("--batch-slice needs --batch-size")
    if args.batch_slice is None:
        args.batch_slice = "torch"
    if "ms_academic" in args.dataset:  # main.py:56-59
        args.alpha = 0.2
        args.nknown = 5000
    return args


def main(argv=None):
    args = parse_args(argv)
    set_seeds(args.seed)
    device = torch.device("cuda")
    adj, attr, labels = load_dataset(args.dataset)
    records, builds, coefs = [], [], []
    for _ in range(args.n_runs):
        stats = {}
        rec = run_once(adj, attr, labels, args, device, stats)
        builds.append(stats.get("ppr_build", 0.0))
        if "coef" in stats:
            coefs.append(stats["coef"])
        print(rec, flush=True)
        records.append(rec)
    acc = np.array([r["valid_acc"] for r in records])
    summary = {"dataset": args.dataset, "model": args.model, "K": args.K, "runs": len(acc),
               "valid_acc_mean": float(acc.mean()), "valid_acc_std": float(acc.std(ddof=1))
               if len(acc) > 1 else 0.0,
               "epochs_mean": float(np.mean([r["epoch"] for r in records])),
               "elapsed_mean": float(np.mean([r["elapsed"] for r in records]))}
    if coefs:
        summary.update({"coef_init": args.coef_init, "learn_coef": not args.fixed_coef,
                        "coef": coefs})
    if args.batch_size:
        if args.ppr_eps is not None:
            summary["ppr_eps"] = args.ppr_eps
            summary["ppr_select"] = args.ppr_select
        summary.update({"batch_size": args.batch_size, "ppr_topk": args.ppr_topk,
                        "batch_slice": args.batch_slice,
                        "ppr_build_mean": float(np.mean(builds)),
                        "records": records})
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
