"""train.py -- `python train.py --config configs/X.yaml`, the reference's training CLI (ref:train.py:14-101) on the
MI355X-native hot path.

Same flags and YAML keys as the reference: with --config every hyper-parameter comes from the YAML
(experiment, batch_size, d_model, dim_feedforward, dropout, optimizer_algorithm, learning_rate, n_heads,
num_encoder_decoder_layers, epochs, encoder_only, hit_loss_penalty, load_model); without it from the CLI.
The reference's own YAMLs (InfillingClosedHH / KicksAndSnares / Random ...) load unchanged.

Host side stays Python: data come from (a) the reference's processed dataset when its dataset modules are
importable (`load_processed_dataset`, ref:train.py:153-155), (b) --data-npz FILE with arrays
`inputs (N,32,S)` / `outputs (N,32,27)` (= the dataset's processed_inputs/processed_outputs tensors,
ref:dataset.py:263-264), (c) --synthetic N sequences from the SURVEY 8(d) generator, or (d), for the symbolic
infilling experiments, --infill-npz FILE with ONE array `hvo (N,32,27)` of full grooves: the voices to remove are
drawn on the device at every visit (--infill_voices / --infill_min / --infill_max / --infill_prob), or, with --infill_mode events,
a random share of the individual hits (--infill_ratio LO,HI: the reference's InfillingRandom pairing).  W&B is optional.
Data-parallel: launch with torch.distributed.run, one process per GPU.
"""
import argparse
import os
import pprint
import sys
import time

import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

KEYS = ("encoder_only", "optimizer_algorithm", "d_model", "n_heads", "dropout", "num_encoder_decoder_layers",
        "hit_loss_penalty", "batch_size", "dim_feedforward", "learning_rate", "epochs", "load_model")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--paths", default="configs/paths.yaml", help="paths file (experiment -> dataset dirs)")
    p.add_argument("--testing", default=False, help="testing mode (1 epoch)")
    p.add_argument("--wandb", default=True, help="log to wandb (when installed)")
    p.add_argument("--only_final_eval", default=False)
    # which sets are scored per epoch and whether the scores are dumped (ref:train.py:18-24, 219-250).  The reference's
    # GrooveEvaluator (host-side plots / audio, un-vendored) is outside the hot path; its SCALAR leg -- predict the set,
    # per-voice hit accuracy / velocity / offset errors (ref:evaluator.py:516-525) -- runs here on the device
    # (transformergrooveinfilling_amd.metrics.evaluate: chunked predict + gt_voice_metrics, ONE 30-float D2H per set) on the epochs of
    # the reference's save schedule, logged under the reference's set identifiers (Train_Set / Test_Set / Validation_Set).
    p.add_argument("--eval_train", default=True, help="evaluator train set")
    p.add_argument("--eval_test", default=False, help="evaluator test set")
    p.add_argument("--eval_validation", default=True, help="evaluator validation set")
    p.add_argument("--dump_eval", default=True, help="dump the per-epoch evaluation scalars (eval_<Set>_Epoch_<n>.json beside the checkpoints)")
    p.add_argument("--load_model", default=None)
    p.add_argument("--notes", default=None)
    p.add_argument("--tags", default=None)
    p.add_argument("--config", default=None, help="yaml config file; if given the hyper-parameter flags are ignored")
    p.add_argument("--experiment", default=None)
    p.add_argument("--encoder_only", default=1, type=int)
    p.add_argument("--optimizer_algorithm", default="sgd", type=str, help="sgd | adam (ref:train.py:40-42) | adamw")
    p.add_argument("--d_model", default=64, type=int)
    p.add_argument("--n_heads", default=16, type=int)
    p.add_argument("--dropout", default=0.2, type=float)
    p.add_argument("--num_encoder_decoder_layers", default=7, type=int)
    p.add_argument("--hit_loss_penalty", default=1, type=float)
    p.add_argument("--batch_size", default=16, type=int)
    p.add_argument("--dim_feedforward", default=256, type=int)
    p.add_argument("--learning_rate", default=0.05, type=float)
    p.add_argument("--epochs", default=100, type=int)
    # build-side additions
    p.add_argument("--data-npz", default=None, help="npz with inputs (N,32,S) and outputs (N,32,27)")
    p.add_argument("--synthetic", default=0, type=int, help="train on N synthetic sequences")
    p.add_argument("--eval-npz", default=None,
                   help="npz with the evaluation subsets: train_inputs/train_gt, test_inputs/test_gt, validation_inputs/validation_gt "
                        "((n,32,S) / (n,32,27): the evaluators' processed_inputs / processed_gt, ref:evaluator.py:509-511); missing sets are "
                        "skipped.  With --synthetic and no file: three seeded synthetic subsets.  Genre tags: <set>_groups (n integers; the keys "
                        "are train_groups, test_groups, validation_groups) and group_names (strings; default group<k>) make the evaluation leg "
                        "also report every metric per group (gt_group_metrics; at most 64 groups)")
    p.add_argument("--eval-size", default=1024, type=int, help="sequences per synthetic / train-derived evaluation subset")
    p.add_argument("--host-loader", action="store_true",
                   help="feed batches through torch's DataLoader from host memory (the reference's way) instead of keeping the "
                        "dataset in HBM and gathering batches on the device")
    p.add_argument("--watch-log-freq", type=int, default=1000, help="gradient histograms to wandb every N batches (ref:train.py:150 wandb.watch log_freq; 0 = off)")
    p.add_argument("--save-dir", default=None, help="where checkpoints go (default: wandb run dir or ./checkpoints)")
    p.add_argument("--override", action="append", default=[], metavar="KEY=VALUE", help="override a YAML key (bench shapes)")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "autocast"],
                   help="bf16: the Linear GEMMs take bf16 operands on the matrix cores (fp32 accumulate, fp32 master weights; BASELINE configs[4]); "
                        "autocast: ... and the encoder layers' Linear outputs are stored in bf16 (gt_config.precision = 2: what torch.autocast keeps in bf16)")
    p.add_argument("--max_grad_norm", default=None, type=float,
                   help="clip the gradients to this global 2-norm every step (torch.nn.utils.clip_grad_norm_; inf: only log the norm as "
                        "train/grad_norm).  Also the YAML key max_grad_norm; the reference does not clip (default: off)")
    p.add_argument("--momentum", default=0.0, type=float, help="SGD momentum (torch.optim.SGD, dampening 0).  Also the YAML key momentum; the reference trains without (default 0)")
    p.add_argument("--nesterov", action="store_true", help="Nesterov momentum (needs --momentum > 0).  Also the YAML key nesterov")
    p.add_argument("--weight_decay", default=None, type=float,
                   help="weight decay: L2 for sgd / adam (added to the gradient), decoupled for adamw.  Also the YAML key weight_decay; "
                        "default: torch's (0; 1e-2 for adamw)")
    # the loss's options (gt_loss_opts; the reference has hit_loss_penalty alone).  Also YAML keys of the same names; all off by default
    p.add_argument("--pos_weight", default=None, type=str, help="BCEWithLogitsLoss(pos_weight): 1 or 9 comma-separated floats (one per voice)")
    p.add_argument("--voice_weight", default=None, type=str, help="9 comma-separated weights, one per voice, on all three loss terms")
    p.add_argument("--focal_gamma", default=None, type=float, help="focal modulation (1 - p_t)^gamma of the hit term, 0..8")
    p.add_argument("--vo_penalty", default=None, type=float, help="penalty of the velocity / offset terms where there is no hit (default: hit_loss_penalty)")
    p.add_argument("--loss_weights", default=None, type=str, help="h,v,o: weights of the hit / velocity / offset terms in the loss")
    # infilling pairs drawn on the device from full grooves (gt_gather_infill; the reference freezes a few voice combinations per groove at
    # preprocessing time, ref:utils.py:69-115).  Also YAML keys of the same names (infill_npz, infill_voices, ...); symbolic experiments only
    p.add_argument("--infill-npz", default=None, help="npz with hvo (N,32,27): full grooves; x / y pairs are drawn on the device every step")
    p.add_argument("--infill_voices", default=None, type=str, help="comma list of the voices that may be removed (voices_params voice_idx; default 2: the closed hi-hat)")
    p.add_argument("--infill_min", default=None, type=int, help="fewest voices removed per groove (default 1)")
    p.add_argument("--infill_max", default=None, type=int, help="most voices removed per groove (default: infill_min)")
    p.add_argument("--infill_prob", default=None, type=str,
                   help="comma list of integer weights, one per size infill_min..infill_max: the weight of EACH combination of that size (default all 1)")
    # per-voice hit thresholds from the threshold curves of the validation set (gt_hit_curve / gt_hit_thresholds).  Also YAML keys; off by default
    p.add_argument("--calibrate_thresholds", default="off", choices=["off", "f_beta", "density"],
                   help="on the evaluation epochs, rank 0 calibrates a hit threshold per voice on Validation_Set (Train_Set when that is "
                        "disabled): f_beta = the best F-beta, density = as many hits as the ground truth; adds hit precision / recall / F1 at "
                        "those thresholds to each set's record, writes voice_thresholds_Epoch_<n>.json, and checkpoints carry the thresholds")
    p.add_argument("--calibrate_beta", default=1.0, type=float, help="the beta of --calibrate_thresholds f_beta (and of the reported F score)")
    # the descriptor leg of the evaluation (gt_groove_features).  Also the YAML key eval_descriptors; off by default
    p.add_argument("--eval_descriptors", default=False,
                   help="on the full-evaluation epochs of the save schedule, write the table of rhythmic descriptors of each evaluated set -- ground "
                        "truth beside prediction, with per-sequence rhythmic distances -- as stats_<Set>_<run id>_Epoch_<n>.csv (per group of a "
                        "tagged set: stats_<Set>_groups_Epoch_<n>.json)")
    p.add_argument("--infill_mode", default=None, choices=["voices", "events"],
                   help="what --infill-npz removes from a groove: voices (default; whole voices, gt_gather_infill) or events (a random share of the "
                        "individual hits across the --infill_voices, default all nine: GrooveMidiDatasetInfillingRandom's pairing, gt_gather_infill_events)")
    p.add_argument("--infill_ratio", default=None, type=str,
                   help="events mode: LO,HI -- the share of the removable hits to take out, drawn per groove and visit (default 0.4,0.6, the reference's thres_range)")
    p.add_argument("--deterministic", action="store_true",
                   help="bitwise-reproducible weight gradients (gt_set_deterministic: no token split in the weight-gradient kernels; +9-30 %% step time)")
    return p


def load_hyperparameters(args):
    """All from the YAML or all from the CLI (ref:train.py:69-96)."""
    if args.config is not None:
        with open(args.config, "r") as f:
            hp = yaml.safe_load(f)
    else:
        hp = {k: getattr(args, k) for k in KEYS}
    if args.testing:
        hp["epochs"] = 1
    if args.experiment is not None:
        hp["experiment"] = args.experiment
    for kv in args.override:
        k, v = kv.split("=", 1)
        hp[k] = yaml.safe_load(v)
    assert "experiment" in hp, "experiment not specified"
    hp.setdefault("load_model", None)          # InfillingRandom_test_large.yaml lacks the key
    # gradient clipping: the YAML key, else --max_grad_norm (the reference's YAMLs lack the key: off, as there)
    mgn = hp.get("max_grad_norm", args.max_grad_norm)
    hp["max_grad_norm"] = None if mgn is None else float(mgn)
    # the optimizer's extras, the same way: YAML key, else the flag (the reference's YAMLs lack the keys: plain SGD / Adam, as there)
    hp["momentum"] = float(hp.get("momentum", args.momentum) or 0.0)
    hp["nesterov"] = bool(hp.get("nesterov", args.nesterov))
    wd = hp.get("weight_decay", args.weight_decay)
    hp["weight_decay"] = None if wd is None else float(wd)
    # the loss's options, the same way (a YAML may give a list or a comma-separated string; the reference's YAMLs lack the keys: the plain loss)
    for k, counts in (("pos_weight", (1, 9)), ("voice_weight", (9,)), ("loss_weights", (3,))):
        hp[k] = _floats(hp.get(k, getattr(args, k)), counts, k)
    for k in ("focal_gamma", "vo_penalty"):
        v = hp.get(k, getattr(args, k))
        hp[k] = None if v is None else float(v)
    # threshold calibration, the same way (only where set: with it off the printed / logged hyper-parameters are the reference's)
    cal = str(hp.get("calibrate_thresholds", args.calibrate_thresholds) or "off").lower()
    if cal not in ("off", "false", "f_beta", "density"):
        raise SystemExit("calibrate_thresholds must be off, f_beta or density, got %r" % cal)
    hp.pop("calibrate_thresholds", None)
    cal_beta = float(hp.pop("calibrate_beta", args.calibrate_beta))
    if cal in ("f_beta", "density"):
        if not (0.0 < cal_beta < float("inf")):
            raise SystemExit("calibrate_beta must be > 0 and finite, got %r" % cal_beta)
        hp["calibrate_thresholds"], hp["calibrate_beta"] = cal, cal_beta
    # the descriptor leg, the same way (only where set, as above)
    if _flag(hp.pop("eval_descriptors", args.eval_descriptors)):
        hp["eval_descriptors"] = True
    # infilling from full grooves, the same way
    hp["infill_npz"] = hp.get("infill_npz", args.infill_npz)
    hp["infill"] = infill_setup(hp, args)
    return hp


SYMBOLIC = ("InfillingClosedHH_Symbolic", "InfillingRandom_Symbolic")      # the experiments whose input is an HVO groove (embedding_size_src 27, ref:train.py:129-131)


def _ints(v, what):
    """None, a number, a list or a comma-separated string -> list of ints"""
    if v is None:
        return None
    try:
        v = [a for a in v.split(",")] if isinstance(v, str) else list(v) if hasattr(v, "__len__") else [v]
        if any(float(a) != int(float(a)) for a in v):
            raise ValueError(v)
        return [int(float(a)) for a in v]
    except ValueError:
        raise SystemExit("--%s expects comma-separated integers, got %r" % (what, v))


def infill_setup(hp, args):
    """make_infill_opts keywords of the infill flags / YAML keys, or None while none is given; with infill_mode events, the dict
    infill.as_opts takes for the event options: mode="events" beside make_infill_event_opts keywords.  SystemExit for a non-symbolic
    experiment: only there is the input the groove itself."""
    vals = {k: hp.get(k, getattr(args, k)) for k in ("infill_voices", "infill_min", "infill_max", "infill_prob", "infill_mode", "infill_ratio")}
    if hp.get("infill_npz") is None and all(v is None for v in vals.values()):
        return None
    if hp["experiment"] not in SYMBOLIC:
        raise SystemExit("--infill-npz / --infill_* need a symbolic experiment (%s): the input of %r is not an HVO groove"
                         % (", ".join(SYMBOLIC), hp["experiment"]))
    if hp.get("infill_npz") is None:
        raise SystemExit("--infill_voices / --infill_min / --infill_max / --infill_prob need --infill-npz FILE (full grooves)")
    from transformergrooveinfilling_amd import _lib
    mode = "voices" if vals["infill_mode"] is None else str(vals["infill_mode"])
    if mode not in ("voices", "events"):
        raise SystemExit("infill_mode must be voices or events, got %r" % (mode,))
    if mode == "events":
        given = [k for k in ("infill_min", "infill_max", "infill_prob") if vals[k] is not None]
        if given:
            raise SystemExit("%s select how many whole voices go: they do not apply to --infill_mode events (use --infill_ratio)" % " / ".join(given))
        try:
            ratio = [0.4, 0.6] if vals["infill_ratio"] is None else _floats(vals["infill_ratio"], (2,), "infill_ratio")
        except ValueError:
            raise SystemExit("--infill_ratio expects two comma-separated floats LO,HI, got %r" % (vals["infill_ratio"],))
        kw = dict(mode="events", voices=_ints(vals["infill_voices"], "infill_voices") or list(range(9)), ratio=ratio)
        try:
            _lib.make_infill_event_opts(voices=kw["voices"], ratio=ratio)
        except ValueError as e:
            raise SystemExit("infill options: %s" % e)
        return kw
    if vals["infill_ratio"] is not None:
        raise SystemExit("--infill_ratio is the share of hits --infill_mode events removes: it does not apply to --infill_mode voices")
    lo = 1 if vals["infill_min"] is None else int(vals["infill_min"])
    kw = dict(voices=_ints(vals["infill_voices"], "infill_voices") or [2], min_remove=lo,
              max_remove=lo if vals["infill_max"] is None else int(vals["infill_max"]), prob=_ints(vals["infill_prob"], "infill_prob"))
    try:
        _lib.make_infill_opts(**kw)
    except ValueError as e:
        raise SystemExit("infill options: %s" % e)
    return kw


def _floats(v, counts, what):
    """None, a number, a list or a comma-separated string -> list of floats whose length is one of `counts`"""
    if v is None:
        return None
    v = [float(a) for a in v.split(",")] if isinstance(v, str) else [float(a) for a in v] if hasattr(v, "__len__") else [float(v)]
    if len(v) not in counts:
        raise SystemExit("--%s expects %s comma-separated floats, got %d" % (what, " or ".join(str(c) for c in counts), len(v)))
    return v


def loss_setup(hp):
    """(bce_fn keywords, train_loop's loss_options) of the loss flags / YAML keys: ({}, None) while none is set"""
    opts = {k: hp[src] for k, src in (("voice_weight", "voice_weight"), ("focal_gamma", "focal_gamma"), ("vo_penalty", "vo_penalty"),
                                      ("term_weights", "loss_weights")) if hp.get(src) is not None}
    return ({} if hp.get("pos_weight") is None else {"pos_weight": hp["pos_weight"]}), (opts or None)


def model_params(hp, device):
    """params dict of ref:train.py:115-143."""
    enc_only = bool(hp["encoder_only"])
    # (the optimizer's extras only where set: a reference YAML gives exactly the reference's three training keys)
    extras = {k: hp[k] for k in ("momentum", "nesterov") if hp.get(k)}
    if hp.get("weight_decay") is not None:     # (an explicit 0 counts: adamw's default is torch's 1e-2)
        extras["weight_decay"] = hp["weight_decay"]
    return {"model": {"experiment": hp["experiment"], "encoder_only": hp["encoder_only"], "optimizer": hp["optimizer_algorithm"],
                      "d_model": hp["d_model"], "n_heads": hp["n_heads"], "dim_feedforward": hp["dim_feedforward"],
                      "dropout": hp["dropout"], "num_encoder_layers": hp["num_encoder_decoder_layers"],
                      "num_decoder_layers": 0 if enc_only else hp["num_encoder_decoder_layers"], "max_len": 32,
                      "embedding_size_src": 27 if hp["experiment"] in SYMBOLIC else 16,
                      "embedding_size_tgt": 27, "device": device},
            "training": {"learning_rate": hp["learning_rate"], "batch_size": hp["batch_size"],
                         "hit_loss_penalty": hp["hit_loss_penalty"], **extras},
            "load_model": hp["load_model"]}


def synthetic_tensors(n, src_dim, seed):
    """x ~ U[0,1); hits ~ Bernoulli(0.15), vel = U*h, off = (U-0.5)*h  (SURVEY 8d)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 32, src_dim, generator=g)
    h = (torch.rand(n, 32, 9, generator=g) < 0.15).float()
    v = torch.rand(n, 32, 9, generator=g) * h
    o = (torch.rand(n, 32, 9, generator=g) - 0.5) * h
    return x, torch.cat([h, v, o], -1)


def load_data(args, hp, src_dim):
    import numpy as np
    import torch
    if args.synthetic:
        return synthetic_tensors(args.synthetic, src_dim, args.seed + 1)
    if args.data_npz:
        z = np.load(args.data_npz)
        return torch.from_numpy(z["inputs"]).float(), torch.from_numpy(z["outputs"]).float()
    try:                                    # the reference's own host-side data path, if present on PYTHONPATH
        from process_dataset import load_processed_dataset
    except Exception as e:
        raise SystemExit("no data: pass --synthetic N or --data-npz FILE, or put the reference's dataset modules on "
                         "PYTHONPATH (%s)" % e)
    with open(args.paths, "r") as f:
        paths = yaml.safe_load(f)
    ds = load_processed_dataset(paths[hp["experiment"]]["datasets"]["train"], exp=hp["experiment"])
    return ds.processed_inputs, ds.processed_outputs


def _flag(v):
    """the reference's boolean flags arrive as strings from sweep command lines (`--eval_test False`)"""
    return bool(v) and str(v).lower() not in ("false", "0", "no", "none")


def load_eval_sets(args, x, y, src_dim, pair=None, info=None, x_mask=None):
    """{"Train_Set" | "Test_Set" | "Validation_Set": (inputs, gt)} for the sets the flags enable (ref:train.py:160-174: three
    pickled evaluators, each holding processed_inputs / processed_gt of a subset).  Sources: --eval-npz; else, with --synthetic,
    seeded synthetic subsets; the train subset defaults to the head of the training tensors.  pair (infilling from full grooves): a set given
    as ONE array <set>_hvo (n,32,27) is paired once through it -- a fixed state, so every epoch scores the same pairs; pair returns
    (inputs, gt, mask, kept): what the pairing removed (voice bitmasks or cell words) and the indices of the grooves it could pair.
    info (a dict, filled per set name): "mask" -- that third result (x_mask: the one of the training tensors' own pairing) --, and for a
    set the file tags with <set>_groups: "groups" (n int32), "names", "n_groups" (the largest id + 1; the file's group_names or group<k>).
    SystemExit for tags that do not fit their set or name more than 64 groups."""
    import numpy as np
    import torch
    want = {"Train_Set": _flag(args.eval_train), "Test_Set": _flag(args.eval_test), "Validation_Set": _flag(args.eval_validation)}
    key = {"Train_Set": "train", "Test_Set": "test", "Validation_Set": "validation"}
    sets = {}
    z = np.load(args.eval_npz) if args.eval_npz else None
    info = {} if info is None else info
    for i, (name, on) in enumerate(want.items()):
        if not on:
            continue
        k = key[name]
        kept, from_file = None, False
        if z is not None and k + "_inputs" in z.files:
            sets[name] = (torch.from_numpy(z[k + "_inputs"]).float(), torch.from_numpy(z[k + "_gt"]).float())
            from_file = True
        elif z is not None and pair is not None and k + "_hvo" in z.files:
            xi, gi, mask, kept = pair(torch.from_numpy(z[k + "_hvo"]).float())
            sets[name] = (xi, gi)
            info.setdefault(name, {})["mask"] = mask
            from_file = True
        elif name == "Train_Set":
            n = min(args.eval_size, len(x))
            sets[name] = (x[:n], y[:n])
            if x_mask is not None:
                info.setdefault(name, {})["mask"] = x_mask[:n]
        elif args.synthetic:
            sets[name] = synthetic_tensors(args.eval_size, src_dim, args.seed + 100 + i)
        if from_file and k + "_groups" in z.files:
            g = np.asarray(z[k + "_groups"]).reshape(-1)
            if kept is not None and len(g) == len(z[k + "_hvo"]):
                g = g[kept.numpy()]                      # (the grooves the pairing left out take their tags with them)
            if len(g) != len(sets[name][0]) or not np.issubdtype(g.dtype, np.integer):
                raise SystemExit("--eval-npz: %s_groups must hold one integer tag per sequence (%d), got %d of %s"
                                 % (k, len(sets[name][0]), len(g), g.dtype))
            n_groups = max(1, int(g.max()) + 1)
            if n_groups > 64:
                raise SystemExit("--eval-npz: %s_groups names %d groups; the per-group evaluation takes at most 64 (GT_GM_MAX_GROUPS)" % (k, n_groups))
            names = [str(s) for s in z["group_names"]] if "group_names" in z.files else []
            names = names[:n_groups] + ["group%d" % j for j in range(len(names), n_groups)]
            info.setdefault(name, {}).update(groups=torch.from_numpy(g.astype(np.int32)), names=names, n_groups=n_groups)
    return sets


def write_descriptors(model, name, xin, gt, tagged, infill_kw, gt_records, ep, save_dir, run_id, wb=None):
    """The descriptor table of one evaluated set: stats_<Set>_<run id>_Epoch_<n>.csv (rows: the seven statistics; columns: every descriptor
    as __Ground_Truth and __Prediction, every Distance::<name>), stats_<Set>_groups_Epoch_<n>.json for a tagged set, one printed line, and a
    record of its own on model.eval_log (and W&B).  An infilling run scores the finished groove (model.infill) against the source groove,
    as the Infill_* scalars do; gt_records keeps the target's records per set on the device."""
    import json
    import torch
    from transformergrooveinfilling_amd import metrics
    if infill_kw is not None:
        target = xin + gt
        if infill_kw.get("mode") == "events":
            pred = model.infill(xin, cells=(gt[..., :9] != 0))
        else:
            mask = tagged.get("mask")
            if mask is None:
                mask = ((gt[..., :9] != 0).any(1).to(torch.int32) << torch.arange(9, dtype=torch.int32)).sum(1).to(torch.int32)
            pred = model.infill(xin, removed=mask)
    else:
        target, pred = gt, model.predict_hvo(xin)
    if name not in gt_records:
        gt_records[name] = model.engine.groove_features(target)
    tables = metrics.groove_table(model, pred, target, groups=tagged.get("groups"), names=tagged.get("names"), gt_feat=gt_records[name])
    tab = tables["Overall"]
    cols = [k for k, v in tab.items() if isinstance(v, dict)]
    with open(os.path.join(save_dir, "stats_%s_%s_Epoch_%d.csv" % (name, run_id, ep)), "w") as f:
        f.write(",".join([""] + ['"%s"' % c for c in cols]) + "\n")
        for stat in metrics.TABLE_STATS:
            f.write(",".join([stat] + [repr(tab[c][stat]) for c in cols]) + "\n")
    if "groups" in tagged:
        with open(os.path.join(save_dir, "stats_%s_groups_Epoch_%d.json" % (name, ep)), "w") as f:
            json.dump(dict(tables, epoch=ep, set=name, groups=tagged["names"]), f)
    rec = {}
    for k, v in tab.items():
        if k.startswith("Distance::"):
            rec["%s/Distance/%s_mean" % (name, k[len("Distance::"):])] = v["mean"]
        elif isinstance(v, dict):
            rec["%s/Descriptor/%s_mean" % (name, k)] = v["mean"]
        else:
            rec["%s/Descriptor/%s" % (name, k)] = v
    model.eval_log.append(dict(rec, epoch=ep))
    if wb:
        wb.log(dict(rec, epoch=ep), commit=False)
    print("  %s descriptors: Hamming %.2f  fuzzy %.2f  velocity L2 %.4f  offset RMS %.4f  W1 of NoI %.3f / step density %.4f / velocity mean %.4f" %
          (name, tab["Distance::Hamming"]["mean"], tab["Distance::Fuzzy Hamming"]["mean"], tab["Distance::Velocity L2"]["mean"],
           tab["Distance::Offset RMS"]["mean"], tab["Statistical::NoI__W1"], tab["Statistical::Total Step Density__W1"],
           tab["Statistical::Poly Velocity Mean__W1"]))


def main(argv=None):
    args = build_parser().parse_args(argv)
    hp = load_hyperparameters(args)
    import torch
    from torch.utils.data import DataLoader, TensorDataset
    from transformergrooveinfilling_amd import parallel
    from transformergrooveinfilling_amd import metrics
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model, save_schedule, train_loop
    rank, local, world = parallel.init_distributed()
    if rank == 0:
        pprint.pprint(hp)
    if not torch.cuda.is_available():
        raise SystemExit("train.py runs the MI355X hot path; no ROCm GPU is visible (there is no CPU fallback)")
    device = "cuda:%d" % local
    torch.manual_seed(args.seed)
    wb = None
    if args.wandb and str(args.wandb) != "False" and rank == 0:
        try:
            import wandb as wb
            wb.init(config=hp, project=hp["experiment"], job_type="train", notes=args.notes, tags=args.tags)
        except Exception:
            wb = None
    params = model_params(hp, device)
    params["model"]["precision"] = hp.get("precision", args.precision)
    params["seed"] = args.seed                # dropout stream of this run (the data-parallel rank is mixed in by the model)
    model, optimizer, initial_epoch = initialize_model(params)
    model.eval_log = []                       # the evaluation leg's records (also what the tests read)
    # ref:train.py:150 wandb.watch(model, log_freq=1000): on the fused path the gradients never pass through autograd, so the hooks
    # wandb installs would never fire -- train_loop logs the same "gradients/<name>" histograms itself every watch_log_freq batches
    model.watch_log_freq = args.watch_log_freq if wb is not None else 0
    if args.deterministic:
        model.engine.lib.cdll.gt_set_deterministic(1)
    parallel.broadcast_parameters(model.engine.params)
    infill_kw = hp.get("infill")
    if infill_kw is not None:
        # ONE array of full grooves; training draws the pair on the device at every visit.  What the host-side consumers below need as
        # (x, y) tensors -- the train evaluation subset -- is paired ONCE with a fixed state (step 0, the run's seed) through the same call
        import numpy as np
        from transformergrooveinfilling_amd import infill
        hvo = torch.from_numpy(np.load(hp["infill_npz"])["hvo"]).float()
        if hvo.dim() != 3 or tuple(hvo.shape[1:]) != (32, 27):
            raise SystemExit("--infill-npz: hvo must be (N,32,27), got %s" % (tuple(hvo.shape),))
        if args.host_loader:
            raise SystemExit("--infill-npz draws the pairs on the device: it cannot be combined with --host-loader")
        # (events mode: pair_once_events; its third result is the removed cells, which the evaluation merge below is confined to)
        pair_once = infill.pair_once_events if infill_kw.get("mode") == "events" else infill.pair_once
        x, y, x_mask = (t.cpu() for t in pair_once(hvo[:args.eval_size], infill_kw, seed=args.seed, device=device))
    else:
        x_mask = None
        x, y = load_data(args, hp, params["model"]["embedding_size_src"])

    class _Triples(TensorDataset):           # the reference's dataset yields (x, y, idx) (ref:dataset.py:355-356)
        def __getitem__(self, i):
            return self.tensors[0][i], self.tensors[1][i], i

    ds = _Triples(x, y)
    pair = None
    if infill_kw is not None:
        def pair(h):          # (inputs, gt, what was removed -- voice bitmasks or cell words --, the indices of the grooves that could be paired)
            kept = infill.eligible(h.to(device), infill_kw).cpu()
            return tuple(t.cpu() for t in pair_once(h, infill_kw, seed=args.seed, device=device)) + (kept,)
    eval_info = {}
    eval_sets = load_eval_sets(args, x, y, params["model"]["embedding_size_src"], pair, eval_info, x_mask) if rank == 0 else {}
    test = eval_sets.get("Test_Set", (None, None))
    val = eval_sets.get("Validation_Set", (None, None))
    if infill_kw is not None:
        sampler = loader = parallel.DeviceBatchLoader.infilling(hvo, infill_kw, hp["batch_size"], device, rank, world, seed=args.seed)
        ds = range(loader.n)                  # (only its length is used below: the grooves that can be paired)
    elif not args.host_loader:
        # the whole dataset in HBM, batches gathered on the device
        sampler = loader = parallel.DeviceBatchLoader(x, y, hp["batch_size"], device, rank, world, seed=args.seed)
    elif world > 1:
        sampler = parallel.ShardedBatchSampler(len(ds), hp["batch_size"], rank, world, seed=args.seed)
        loader = DataLoader(ds, batch_sampler=sampler, pin_memory=True)
    else:
        sampler = None
        loader = DataLoader(ds, batch_size=hp["batch_size"], shuffle=True, pin_memory=True)
    bce_kw, loss_options = loss_setup(hp)
    bce_kw = {k: torch.tensor(v, device=device) for k, v in bce_kw.items()}
    bce, mse = torch.nn.BCEWithLogitsLoss(reduction="none", **bce_kw), torch.nn.MSELoss(reduction="none")
    gt_records = {}                           # --eval_descriptors: the ground truth's records per set, computed once, kept on the device
    part, full = save_schedule(hp["epochs"], only_final=bool(args.only_final_eval) and str(args.only_final_eval) != "False")
    save_dir = args.save_dir or (wb.run.dir if wb else os.path.join(ROOT, "checkpoints"))
    os.makedirs(save_dir, exist_ok=True)
    for ep in range(initial_epoch, hp["epochs"]):
        if sampler:
            sampler.set_epoch(ep)
        t0 = time.perf_counter()
        m = train_loop(dataloader=loader, groove_transformer=model, encoder_only=hp["encoder_only"], opt=optimizer, epoch=ep,
                       loss_fn=calculate_loss, bce_fn=bce, mse_fn=mse, device=device, hit_loss_penalty=hp["hit_loss_penalty"],
                       # test / validation LOSS after the epoch's batches, as the reference's train_loop arguments (ref:train.py:204-212)
                       test_inputs=test[0], test_gt=test[1], validation_inputs=val[0], validation_gt=val[1],
                       save=(rank == 0 and (ep in part or ep in full)), save_dir=save_dir,
                       run_id=(wb.run.id if wb else "local"), max_grad_norm=hp["max_grad_norm"], loss_options=loss_options)
        torch.cuda.synchronize()
        if rank == 0:
            n = min(len(loader) * hp["batch_size"], len(ds) // world) * world
            print("Epoch %d: loss %.5f  hit_acc %.4f  (%.0f sequences/s)" % (ep, m["train/loss"], m["train/hit_accuracy"],
                                                                           n / (time.perf_counter() - t0)))
            # the evaluation leg (ref:train.py:219-250 -> log_eval, ref:evaluator.py:516-525) on the epochs of the save schedule:
            # predict each enabled set on the device, per-voice metrics on the device, one 30-float copy per set
            if ep in part or ep in full:
                cal = hp.get("calibrate_thresholds")
                cal_set = next((s for s in ("Validation_Set", "Train_Set") if s in eval_sets), None)
                if cal and cal_set:
                    # thresholds per voice from the threshold curves of the validation set (counted on the device, one copy of the counts);
                    # they stay on the model: the checkpoints written from here on carry them
                    import json
                    res = model.calibrate_thresholds(*eval_sets[cal_set], criterion=cal, beta=hp["calibrate_beta"])
                    print("  calibrated hit thresholds (%s on %s): %s" % (cal, cal_set, " ".join("%.2f" % t for t in res["thresholds"])))
                    with open(os.path.join(save_dir, "voice_thresholds_Epoch_%d.json" % ep), "w") as f:
                        json.dump({"epoch": ep, "criterion": cal, "beta": hp["calibrate_beta"], "set": cal_set, "voices": list(metrics.VOICES),
                                   "thresholds": res["thresholds"], "index": res["index"],
                                   **{k: res[k] for k in ("precision", "recall", "f_beta", "density_ratio")}}, f)
                for name, (xin, gt) in eval_sets.items():
                    sc = metrics.evaluate(model, xin, gt)
                    tagged = eval_info.get(name, {})
                    grec, glines = {}, []
                    if "groups" in tagged:
                        # the reference's per-subset numbers (ref:evaluator.py:171-196): the same predictions counted per genre tag on the device
                        by_group = metrics.evaluate_groups(model, xin, gt, tagged["groups"], names=tagged["names"])
                        for gname in tagged["names"]:
                            gs = by_group[gname]
                            glines.append("    %s / %s: %d sequences  hits F1 %.4f  accuracy %.4f  velocity MSE on hits %.5f  offset MSE on hits %.5f" %
                                          (name, gname, gs["Sequences"], gs["Hits_F1_Overall"], gs["Hits_Accuracy_Overall"],
                                           gs["Velocity_MSE_Hits_Overall"], gs["Offset_MSE_Hits_Overall"]))
                            grec.update({"%s/%s/%s" % (name, gname, k): v for k, v in gs.items()})
                    if infill_kw is not None and infill_kw.get("mode") == "events":
                        # the finished groove against the source groove: the prediction merged into its input, confined to the removed
                        # cells (gt_infill_merge_cells) -- they are the cells where the target has a hit
                        done = model.infill(xin, cells=(gt[..., :9] != 0))
                        sc.update({"Infill_" + k: v for k, v in metrics.voice_metrics(model, done, xin + gt).items()})
                        # ... and counted over those cells alone: everywhere else the finished groove is the source by construction
                        removed_part = metrics.group_metrics(model, done, xin + gt, cells=(gt[..., :9] != 0))["Overall"]
                        sc.update({"Infill_Removed_" + k: v for k, v in removed_part.items()})
                    elif infill_kw is not None:
                        # voices mode: the removed part is whole voices -- the pairing's bitmasks; a set that arrived already paired has them in
                        # its target, which keeps the removed voices alone (only voices with a hit are ever removed)
                        mask = tagged.get("mask")
                        if mask is None:
                            mask = ((gt[..., :9] != 0).any(1).to(torch.int32) << torch.arange(9, dtype=torch.int32)).sum(1).to(torch.int32)
                        done = model.infill(xin, removed=mask)
                        removed_part = metrics.group_metrics(model, done, xin + gt, removed=mask)["Overall"]
                        sc.update({"Infill_Removed_" + k: v for k, v in removed_part.items()})
                    if cal and cal_set:
                        sc.update(metrics.hit_scores(model, xin, gt, voice_thresholds="calibrated", beta=hp["calibrate_beta"]))
                    rec = {"%s/%s" % (name, k): v for k, v in sc.items()}
                    rec.update(grec)
                    model.eval_log.append(dict(rec, epoch=ep))
                    print("  %s: hits accuracy %.4f  velocity MSE %.5f  offset MSE %.5f" %
                          (name, sc["Hits_Accuracy_Overall"], sc["Velocity_MSE_Overall"], sc["Offset_MSE_Overall"]))
                    for line in glines:                 # one line per group of a tagged set
                        print(line)
                    if wb:
                        wb.log(dict(rec, epoch=ep), commit=False)
                    if _flag(args.dump_eval):
                        import json
                        with open(os.path.join(save_dir, "eval_%s_Epoch_%d.json" % (name, ep)), "w") as f:
                            json.dump(dict(sc, epoch=ep), f)
                        if "groups" in tagged:
                            with open(os.path.join(save_dir, "eval_%s_groups_Epoch_%d.json" % (name, ep)), "w") as f:
                                json.dump(dict(by_group, epoch=ep, set=name, groups=tagged["names"]), f)
            # the descriptor leg (the second leg of ref:evaluator.py:516-601, get_stats_from_evaluator's table on the "all" epochs): the
            # records of every sequence on the device (gt_groove_features), one copy per set, the table on the host
            if hp.get("eval_descriptors") and ep in full:
                for name, (xin, gt) in eval_sets.items():
                    write_descriptors(model, name, xin, gt, eval_info.get(name, {}), infill_kw, gt_records, ep, save_dir,
                                      wb.run.id if wb else "local", wb)
            if wb:
                wb.log({"epoch": ep}, commit=True)
    if wb:
        wb.finish()
    return model


if __name__ == "__main__":
    main()
