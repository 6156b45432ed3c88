"""Command-line surface of ``T/parameters.py`` (same flags and defaults) plus what the reference forgot or
what ROCm / torchrun need: ``--news`` (read by ``T/run.py:79,100`` but never declared), ``--local-rank`` (torch >= 2.0
launcher spelling), and the MI355X-path switches."""
import argparse
import os
import sys


ITEM_TOWERS = ("id", "modal", "modal_add", "modal_cat", "modal_cat_3")


def build_parser():
    p = argparse.ArgumentParser()
    # ============== data_dir ==============
    p.add_argument("--mode", type=str, default="train")
    p.add_argument("--item_tower", type=str, default="id", choices=ITEM_TOWERS,
                   help="id | modal, or ID (+) modality fusion (bce_text/id_plus_mo-end2end): modal_add = id vector + content vector, "
                        "modal_cat / modal_cat_3 = their concatenation through one / three Dropout-Linear-GELU layers")
    p.add_argument("--arch", type=str, default="sasrec", choices=["sasrec", "dssm", "two_stage", "id_two_stage"],
                   help="sasrec = the sequential user encoder (everything as before); dssm = the two-tower model of "
                        "bce_text/main-end2end(DSSM): user-id embedding + MLP against 1 + neg_num sampled items per (user, item) pair, "
                        "BCE loss; --item_tower id | modal (text), autograd path; --loss is not consulted; two_stage = "
                        "bce_text|bce_vision/main-2stage(SASRec): the item tower runs once over the catalogue (or --features_npy supplies its "
                        "features), an MLP over the frozen feature rows + SASRec + BCE are trained; --item_tower modal, autograd path; "
                        "id_two_stage = bce_text|bce_vision/id_plus_mo-2stage: the same frozen features fused with a trained id table, "
                        "--item_tower modal_add | modal_cat, --mo_dnn_layers / --dnn_layers")
    p.add_argument("--neg_num", type=int, default=1, help="--arch dssm: sampled negatives per (user, item) pair")
    p.add_argument("--dnn_layers", type=int, default=0, help="--arch dssm: Dropout-Linear-GELU layers of the user MLP and of the ID tower's item "
                   "MLP; --arch id_two_stage: Dropout-Linear-GELU layers behind the fusion")
    p.add_argument("--mo_dnn_layers", type=int, default=0, help="--arch id_two_stage: Dropout-Linear-GELU layers between the feature projection "
                   "and the fusion (0: lookup, projection and fusion run as one kernel)")
    p.add_argument("--dnn_layer", type=int, default=0, help="--arch two_stage: Dropout-Linear-GELU layers behind fc (the reference's spelling)")
    p.add_argument("--features_npy", type=str, default="None", help="--arch two_stage: fp16 / fp32 [item_num + 1, W] item features from any "
                   "encoder (row 0 = padding item); skips stage 1")
    p.add_argument("--save_features", type=str, default="None", help="--arch two_stage: write the feature table stage 1 extracted to this .npy file")
    p.add_argument("--root_data_dir", type=str, default="../")
    p.add_argument("--dataset", type=str, default="MIND-small")
    p.add_argument("--behaviors", type=str, default="behaviors_l5_tr_v.tsv")
    p.add_argument("--news", type=str, default="news.tsv")
    # ============== train parameters ==============
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--epoch", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--fine_tune_lr", type=float, default=1e-5)
    p.add_argument("--l2_weight", type=float, default=0)
    p.add_argument("--fine_tune_l2_weight", type=float, default=0)
    p.add_argument("--drop_rate", type=float, default=0.1)
    # ============== model parameters ==============
    p.add_argument("--bert_model_load", type=str, default="bert-base-uncased")
    p.add_argument("--freeze_paras_before", type=int, default=165)
    p.add_argument("--word_embedding_dim", type=int, default=768)
    p.add_argument("--embedding_dim", type=int, default=256)
    p.add_argument("--num_attention_heads", type=int, default=2)
    p.add_argument("--transformer_block", type=int, default=2)
    p.add_argument("--max_seq_len", type=int, default=20)
    p.add_argument("--min_seq_len", type=int, default=5)
    # ============== switch and logging setting ==============
    p.add_argument("--num_workers", type=int, default=12)
    p.add_argument("--load_ckpt_name", type=str, default="None")
    p.add_argument("--label_screen", type=str, default="None")
    p.add_argument("--logging_num", type=int, default=8)
    p.add_argument("--testing_num", type=int, default=1)
    p.add_argument("--local_rank", "--local-rank", dest="local_rank", default=int(os.environ.get("LOCAL_RANK", -1)), type=int)
    # ============== news information ==============
    p.add_argument("--num_words_title", type=int, default=30)
    p.add_argument("--num_words_abstract", type=int, default=50)
    p.add_argument("--num_words_body", type=int, default=50)
    p.add_argument("--news_attributes", type=str, default="title")
    # ============== vision variant (V/parameters.py:34-39) ==============
    p.add_argument("--CV_model_load", type=str, default="None", help="swin_tiny | swin_small | swin_base, mae_base | mae_large (a name with 'mae' "
                   "or 'checkpoint': the MAE / ViT tower of V/model/model.py:28), or resnet18 | 34 | 50 | 101 | 152 (a name with 'resnet', 'resnet-50' too: the "
                   "ResNet tower of V/model/model.py:24), or beit_base | beit_large | beit_micro (a name with 'beit': "
                   "V/model/model.py:26) (vision item tower)")
    p.add_argument("--mae_mask_ratio", type=float, default=None, help="MAE tower: share of the patches masked in a training forward "
                   "(default: the model's, 0.75)")
    p.add_argument("--mae_eval_mask_ratio", type=float, default=None, help="MAE tower: the same in evaluation mode (catalogue passes); default: "
                   "the training value, as the reference (ViTMAEModel masks at evaluation too); 0 encodes the catalogue from all patches")
    p.add_argument("--CV_resize", type=int, default=224)
    p.add_argument("--image_lmdb", type=str, default="None", help="LMDB of pickled LMDB_Image records (dataset/HM/build_lmdb_hm.py; "
                   "V/parameters.py --lmdb_data): decoded per batch, resized on the GPU; needs the optional `lmdb` module")
    p.add_argument("--images_npy", type=str, default="None",
                   help="uint8 array [item_num + 1, R, R, 3] of decoded, resized item images (row 0 = padding item); stands in for the "
                        "LMDB reader of V/data_utils/dataset.py, whose lmdb / torchvision dependencies are not part of this package")
    p.add_argument("--images_on_device", action="store_true",
                   help="vision towers: upload the image catalogue (--images_npy, the synthetic array or --image_lmdb) to the device once "
                        "(every rank its own copy); a training batch is then its item ids and the towers' first kernels read the pixels "
                        "through them (data_utils.images.DeviceImageCatalogue); the catalogue pass at evaluation reads device views")
    # ============== cold-start / new-item evaluation (V/parameters.py:16-19; data_utils/special.py) ==============
    p.add_argument("--cold_seqs", type=str, default="None", help="--mode test: user lines whose target is a cold item (evaluated after "
                   "the test split); with --synthetic N, a path that does not exist yet is written with synthetic lines")
    p.add_argument("--new_seqs", type=str, default="None", help="--mode test, modal towers: user lines whose last item is a NEW item")
    p.add_argument("--new_items", type=str, default="None", help="vision: the new items' names (v<int>), one per line; their order = ids")
    p.add_argument("--new_lmdb_data", type=str, default="None", help="vision: LMDB of the new items' images (needs the optional `lmdb` module)")
    p.add_argument("--new_images_npy", type=str, default="None",
                   help="vision: uint8 [n_new + 1, R, R, 3] images of the new items (row 0 unused); stands in for --new_lmdb_data as "
                        "--images_npy does for the catalogue")
    # ============== recommendation lists (data_utils/metrics.py: recommend_users) ==============
    p.add_argument("--topk", type=int, default=10, help="--mode recommend: items per user (at most the top-K kernel's cap)")
    p.add_argument("--recommend_out", type=str, default="None", help="--mode recommend: output file, one line per test user "
                   "(<user>\\t<item>:<score> ...); default: recommend_top<K>.tsv in the run's checkpoint directory")
    # ============== MI355X path ==============
    p.add_argument("--compute_dtype", type=str, default="fp16", choices=["bf16", "fp16", "fp32", "fp32x3", "fp16_res32", "bf16_res32"],
                   help="fp16 (default) = IEEE half operands on the MFMA, fp32 accumulate, with the reference's GradScaler loss scaling -- the arithmetic of "
                        "its own autocast step (T/run.py:210,242-247; V/run.py likewise) and what bench.py times; bf16 = the same kernels on bf16 operands, no "
                        "loss scaling; fp32 = exact-fp32 MFMA parity mode; fp32x3 = fp32 tensors with every GEMM as three bf16 MFMA passes over hi / lo "
                        "operand splits (fp32 nn.Linear numerics to ~1e-5); fp16_res32 / bf16_res32 = 16-bit GEMMs with an fp32 residual stream "
                        "(LayerNorm in and out fp32): the data flow of torch.cuda.amp.autocast itself, text / ID towers")
    p.add_argument("--pool_negatives", action="store_true", help="pool in-batch negatives over ranks (RCCL all-gather)")
    p.add_argument("--sync_bn", action="store_true",
                   help="torch.nn.SyncBatchNorm.convert_sync_batchnorm(model) before the DDP wrap, as V/run.py:98 does unconditionally: the ResNet "
                   "item tower then takes its BatchNorm statistics over every rank's rows (required for it at a world size above 1); a no-op "
                   "at world size 1 and for every tower without BatchNorm layers")
    p.add_argument("--fused_step", action="store_true",
                   help="flat-arena TrainStep (fused AdamW, one gradient all-reduce) instead of DDP + torch.optim.AdamW")
    p.add_argument("--loss", type=str, default="inbatch", choices=["inbatch", "bce"],
                   help="inbatch = debiased in-batch softmax CE (inbatch_sasrec_e2e_*); bce = one sampled negative per position "
                        "(bce_text/main-end2end; drop-in autograd path only)")
    p.add_argument("--synthetic", type=int, default=0, help="N > 0: train on N synthetic MIND-shaped users (no data files)")
    p.add_argument("--synthetic_items", type=int, default=20000)
    p.add_argument("--synthetic_full_len", action="store_true", help="synthetic users all have raw history max_seq_len + 3 (train sequences "
                   "of exactly S + 1 items, no padding): the shape bench.py times (SURVEY.md §8d)")
    p.add_argument("--max_steps", type=int, default=0)
    p.add_argument("--collate_workers", type=int, default=2, help="worker PROCESSES that build the batches (collate + unpadded-layout index vectors) "
                   "through torch's DataLoader with pin_memory, as T/run.py:111-124 does with num_workers=12 -- no GIL shared with the thread that "
                   "launches ~700 kernels per step; 0 = the in-process collate thread (--prefetch)")
    p.add_argument("--prefetch", type=int, default=4, help="batches built ahead of the device by the collate thread (run.BatchPrefetcher; "
                   "T/run.py:111-124 uses DataLoader(num_workers=12, pin_memory=True)); 0 = collate inline on the main thread")
    p.add_argument("--graph", action="store_true", help="--fused_step on one rank: replay the step as a captured hipGraph per input shape "
                   "(TrainStep.step_graphed; unpadded token rows padded to buckets of 512) instead of host launches")
    p.add_argument("--steady_after", type=int, default=10, help="the epoch log also reports user-seq/s over the steps after this many (allocator "
                   "warm-up, first-call set-up and the loss scaler's initial back-off excluded)")
    p.add_argument("--max_grad_norm", type=float, default=0.0, help="global-norm gradient clipping over all parameter groups together "
                   "(torch.nn.utils.clip_grad_norm_; --fused_step: decided on the device); 0 = off")
    p.add_argument("--lr_schedule", type=str, default="constant", choices=["constant", "linear", "cosine"],
                   help="LR multiplier shared by all parameter groups: 1 (constant), or a linear / cosine decay to --min_lr_ratio at "
                        "epochs x steps-per-epoch, each after --warmup_steps of linear warmup; counted in APPLIED steps")
    p.add_argument("--warmup_steps", type=int, default=0, help="linear LR warmup from 0 over this many applied optimizer steps; 0 = none")
    p.add_argument("--min_lr_ratio", type=float, default=0.0, help="--lr_schedule linear | cosine: the multiplier the decay ends at (and holds)")
    p.add_argument("--checkpoint_root", type=str, default="./checkpoint", help="parent of checkpoint_<tower>.../cpt_<label>/ (T/run.py:326-331)")
    p.add_argument("--pretrained_dir", type=str, default="../pretrained_models",
                   help="directory holding <bert_model_load>/pytorch_model.bin (T/run.py:29-53 reads ../../pretrained_models/)")
    return p


def check_fusion_args(args):
    """What an ID (+) modality fusion tower does not run with: exits with the reason (before anything touches a device)."""
    from .model.encoders import fusion_tower
    kind = fusion_tower(args)[0] if "modal" in str(args.item_tower) else None
    if kind is None:
        return None
    if getattr(args, "fused_step", False) or getattr(args, "graph", False):
        raise SystemExit(f"--item_tower {args.item_tower}: the fusion towers run on the drop-in autograd path (Model / BceModel with "
                         "torch.optim.AdamW); --fused_step / --graph (train_step.TrainStep) do not cover them")
    if getattr(args, "new_seqs", "None") != "None":
        raise SystemExit(f"--item_tower {args.item_tower}: a new item has no row in the id table, so the fused vector fc(id, content) "
                         "does not exist for it; --new_seqs is not available with a fusion tower (--cold_seqs alone is)")
    return kind


def is_mae_run(args) -> bool:
    """A run whose item tower is the MAE (ViT) tower: a modal tower with a ``--CV_model_load`` the reference routes to ``MAE_Encoder``."""
    cv = str(getattr(args, "CV_model_load", "None"))
    return "modal" in str(args.item_tower) and cv != "None" and "swin" not in cv and ("mae" in cv or "checkpoint" in cv)


def check_mae_args(args):
    """What the MAE tower does not run with: exits with the reason (before anything touches a device).  True for an MAE run."""
    if not is_mae_run(args):
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = ("--fused_step" + (" --pool_negatives" if getattr(args, "pool_negatives", False) else "") +
               ": train_step.TrainStep covers the text, ID and Swin towers; the MAE tower trains on the drop-in autograd path")
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which the MAE tower does not use"
    elif getattr(args, "arch", "sasrec") == "dssm":
        why = "--arch dssm: a vision item tower is not built for DSSM"
    for name in ("mae_mask_ratio", "mae_eval_mask_ratio"):
        v = getattr(args, name, None)
        if why is None and v is not None and not 0.0 <= v < 1.0:
            why = f"--{name} must lie in [0, 1)"
    if why:
        raise SystemExit(f"--CV_model_load {args.CV_model_load} (MAE / ViT item tower): " + why)
    return True


def is_beit_run(args) -> bool:
    """A run whose item tower is the BEiT tower: a modal tower with a ``--CV_model_load`` the reference routes to ``Vit_Encoder`` over
    ``BeitForImageClassification`` (``'beit' in CV_model_load``, ``V/model/model.py:26``)."""
    cv = str(getattr(args, "CV_model_load", "None"))
    return "modal" in str(args.item_tower) and "beit" in cv and "swin" not in cv


def check_beit_args(args):
    """What the BEiT tower does not run with: exits with the reason (before anything touches a device).  True for a BEiT run."""
    if not is_beit_run(args):
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = ("--fused_step" + (" --pool_negatives" if getattr(args, "pool_negatives", False) else "") +
               ": train_step.TrainStep covers the text, ID and Swin towers; the BEiT tower trains on the drop-in autograd path")
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which the BEiT tower does not use"
    elif getattr(args, "arch", "sasrec") == "dssm":
        why = "--arch dssm: a vision item tower is not built for DSSM"
    if why:
        raise SystemExit(f"--CV_model_load {args.CV_model_load} (BEiT item tower): " + why)
    return True


def is_resnet_run(args) -> bool:
    """A run whose item tower is the ResNet tower: a modal tower with a ``--CV_model_load`` the reference routes to ``Resnet_Encoder``
    (``'resnet' in CV_model_load``, tested first, ``V/model/model.py:24-25``)."""
    return "modal" in str(args.item_tower) and "resnet" in str(getattr(args, "CV_model_load", "None"))


def check_resnet_args(args):
    """What the ResNet tower does not run with: exits with the reason (before anything touches a device).  True for a ResNet run."""
    if not is_resnet_run(args):
        return False
    import os
    why = None
    tower = str(args.item_tower)
    if getattr(args, "fused_step", False):
        why = ("--fused_step" + (" --pool_negatives" if getattr(args, "pool_negatives", False) else "") +
               ": train_step.TrainStep covers the text, ID and Swin towers; the ResNet tower trains on the drop-in autograd path")
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which the ResNet tower does not use"
    elif getattr(args, "arch", "sasrec") == "dssm":
        why = "--arch dssm: a vision item tower is not built for DSSM"
    elif "add" in tower or "cat" in tower:
        why = f"--item_tower {tower}: the ID + modality fusion towers are not built over the ResNet tower"
    elif int(os.environ.get("WORLD_SIZE", 1)) > 1 and not getattr(args, "sync_bn", False):
        why = ("a world size above 1 needs --sync_bn: the reference converts the tower to SyncBatchNorm (V/run.py:98), and BatchNorm "
               "statistics per rank would silently be another model; --sync_bn converts it and merges the statistics across ranks")
    if why:
        raise SystemExit(f"--CV_model_load {args.CV_model_load} (ResNet item tower): " + why)
    return True


def is_opt_run(args) -> bool:
    """A run whose item tower is the OPT text tower: a modal text tower whose ``--bert_model_load`` the reference routes to ``OPTModel`` /
    ``Text_Encoder_mean`` (``'opt' in bert_model_load``, tested after ``'roberta'``, ``T/run.py:37-47``)."""
    name = str(getattr(args, "bert_model_load", ""))
    return ("modal" in str(args.item_tower) and str(getattr(args, "CV_model_load", "None")) == "None" and "opt" in name
            and "roberta" not in name and "deberta" not in name)


def is_deberta_run(args) -> bool:
    """A run whose item tower is the DeBERTa text tower: a text tower (modal or fusion) whose ``--bert_model_load`` contains 'deberta'
    (``bce_text/main-end2end(DSSM)/run.py:26-31``; tested before 'roberta' and 'opt')."""
    tower = str(args.item_tower)
    text = "modal" in tower or "add" in tower or "cat" in tower
    return text and str(getattr(args, "CV_model_load", "None")) == "None" and "deberta" in str(getattr(args, "bert_model_load", ""))


def check_deberta_args(args):
    """What the DeBERTa tower does not run with: exits with the reason (before anything touches a device).  True for a DeBERTa run."""
    if not is_deberta_run(args):
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = ("--fused_step" + (" --pool_negatives" if getattr(args, "pool_negatives", False) else "") +
               ": train_step.TrainStep covers the BERT / RoBERTa, ID and Swin towers; the DeBERTa tower trains on the drop-in autograd path")
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which the DeBERTa tower does not use"
    if why:
        raise SystemExit(f"--bert_model_load {args.bert_model_load} (DeBERTa text tower): " + why)
    return True


def check_opt_args(args):
    """What the OPT tower does not run with: exits with the reason (before anything touches a device).  True for an OPT run."""
    if not is_opt_run(args):
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = ("--fused_step" + (" --pool_negatives" if getattr(args, "pool_negatives", False) else "") +
               ": train_step.TrainStep covers the BERT / RoBERTa, ID and Swin towers; the OPT tower trains on the drop-in autograd path")
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which the OPT tower does not use"
    elif getattr(args, "arch", "sasrec") == "dssm":
        why = "--arch dssm: the reference's DSSM package has no OPT branch, and none is built"
    if why:
        raise SystemExit(f"--bert_model_load {args.bert_model_load} (OPT text tower): " + why)
    return True


def check_dssm_args(args):
    """What ``--arch dssm`` does not run with: exits with the reason (before anything touches a device).  True for a DSSM run."""
    if getattr(args, "arch", "sasrec") != "dssm":
        return False
    why = None
    if getattr(args, "fused_step", False) or getattr(args, "graph", False):
        why = "--fused_step / --graph (train_step.TrainStep) cover the SASRec models only; DSSM trains on the autograd path"
    elif getattr(args, "pool_negatives", False):
        why = "--pool_negatives pools in-batch negatives; DSSM samples its negatives per pair (--neg_num)"
    elif getattr(args, "mode", "train") == "recommend":
        why = "--mode recommend builds its lists from the sequential user encoder; there is no DSSM form of it"
    elif getattr(args, "cold_seqs", "None") != "None" or getattr(args, "new_seqs", "None") != "None":
        why = "--cold_seqs / --new_seqs evaluate users through their item sequence; a DSSM user is a row of the user table"
    elif args.item_tower not in ("id", "modal"):
        why = f"--item_tower {args.item_tower}: the ID (+) modality fusion towers belong to the SASRec models; DSSM takes id | modal"
    elif getattr(args, "CV_model_load", "None") != "None":
        why = "--CV_model_load: a vision item tower is not built for DSSM (text tower: --item_tower modal with --bert_model_load)"
    elif args.neg_num < 0 or args.dnn_layers < 0:
        why = "--neg_num and --dnn_layers must be >= 0"
    if why:
        raise SystemExit("--arch dssm (DSSM two-tower model): " + why)
    return True


def check_two_stage_args(args):
    """What ``--arch two_stage`` does not run with: exits with the reason (before anything touches a device).  True for a two-stage run."""
    if getattr(args, "arch", "sasrec") != "two_stage":
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = "--fused_step (train_step.TrainStep) covers the end-to-end SASRec models only; two-stage trains on the autograd path"
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which two-stage does not use"
    elif getattr(args, "pool_negatives", False):
        why = "--pool_negatives pools in-batch negatives; two-stage samples one negative per position (BCE)"
    elif getattr(args, "new_seqs", "None") != "None":
        why = "--new_seqs needs the item tower over the new items' content; after stage 1 only the feature table exists (--cold_seqs alone is available)"
    elif args.item_tower != "modal":
        why = (f"--item_tower {args.item_tower}: two-stage trains on frozen MODALITY features (--item_tower modal); the ID (+) modality fusion "
               "towers over frozen features (id_plus_mo-2stage) are --arch id_two_stage")
    elif getattr(args, "loss", "bce") == "inbatch" and getattr(args, "loss_given", False):
        why = "--loss inbatch: the two-stage packages train with the one-sampled-negative BCE loss only"
    elif args.dnn_layer < 0:
        why = "--dnn_layer must be >= 0"
    if why:
        raise SystemExit("--arch two_stage (two-stage training on frozen item features): " + why)
    return True


def check_id_two_stage_args(args):
    """What ``--arch id_two_stage`` does not run with: exits with the reason (before anything touches a device).  True for such a run."""
    if getattr(args, "arch", "sasrec") != "id_two_stage":
        return False
    why = None
    if getattr(args, "fused_step", False):
        why = "--fused_step (train_step.TrainStep) covers the end-to-end SASRec models only; id-two-stage trains on the autograd path"
    elif getattr(args, "graph", False):
        why = "--graph replays the fused step (train_step.TrainStep), which id-two-stage does not use"
    elif getattr(args, "pool_negatives", False):
        why = "--pool_negatives pools in-batch negatives; id-two-stage samples one negative per position (BCE)"
    elif getattr(args, "new_seqs", "None") != "None":
        why = ("--new_seqs: a new item has neither a row in the id table nor, after stage 1, an item tower to encode it "
               "(--cold_seqs alone is available)")
    elif args.item_tower not in ("modal_add", "modal_cat"):
        why = (f"--item_tower {args.item_tower}: the frozen features are fused with the id table through modal_add | modal_cat "
               "(--item_tower modal alone: --arch two_stage; modal_cat_3 is not part of the id_plus_mo-2stage packages)")
    elif getattr(args, "loss", "bce") == "inbatch" and getattr(args, "loss_given", False):
        why = "--loss inbatch: the id_plus_mo-2stage packages train with the one-sampled-negative BCE loss only"
    elif args.mo_dnn_layers < 0 or args.dnn_layers < 0:
        why = "--mo_dnn_layers and --dnn_layers must be >= 0"
    if why:
        raise SystemExit("--arch id_two_stage (id-two-stage: frozen item features fused with a trained id table): " + why)
    return True


def check_images_on_device_args(args):
    """What ``--images_on_device`` does not run with: exits naming the flag (before anything touches a device).  True when it is on."""
    if not getattr(args, "images_on_device", False):
        return False
    why = None
    if "modal" not in args.item_tower:
        why = f"--item_tower {args.item_tower}: the ID tower has no images"
    elif getattr(args, "CV_model_load", "None") == "None":
        why = "a text tower has no images (vision towers: --CV_model_load)"
    elif getattr(args, "graph", False):
        why = "--graph: graph capture of an ids-only vision step is not built"
    elif getattr(args, "arch", "sasrec") != "sasrec":
        why = f"--arch {args.arch}: the device catalogue is built for the end-to-end SASRec models (--loss inbatch | bce)"
    if why:
        raise SystemExit("--images_on_device (image catalogue on the device, batches as item ids): " + why)
    return True


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.news_attributes = args.news_attributes.split(",")
    # --loss defaults to inbatch; --arch two_stage (BCE only) has to tell the default from a request
    args.loss_given = any(a == "--loss" or a.startswith("--loss=") for a in (sys.argv[1:] if argv is None else argv))
    return args
