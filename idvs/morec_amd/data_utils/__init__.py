from .preprocess import read_news, read_news_bert, get_doc_input_bert, read_behaviors, read_images  # noqa: F401
from .dataset import BuildTrainDataset, BuildEvalDataset, SequentialDistributedSampler, collate_train_batch, collate_bce_batch, epoch_batches  # noqa: F401
from .metrics import eval_model, get_item_embeddings  # noqa: F401
from .metrics import PackedEvalUsers, metrics_from_topk, recommend_packed, recommend_users  # noqa: F401
from .special import read_behaviors_special, eval_model_special  # noqa: F401
from .utils import get_checkpoint, load_model, save_model  # noqa: F401
from .images import DeviceImageCatalogue, DeviceImageFeed, ImageIds, LMDB_Image, LmdbImageStore, LmdbItemImages, PatchRows, decode_record, pack_images, resize_table  # noqa: F401
from .dssm import read_behaviors as read_behaviors_dssm, BuildTrainDataset as DssmTrainDataset, eval_model as eval_model_dssm  # noqa: F401
from .dssm import collate_dssm_batch, get_user_embeddings  # noqa: F401
from .two_stage import (collate_two_stage_batch, extract_item_features, get_item_embeddings_id_two_stage,  # noqa: F401
                        get_item_embeddings_two_stage, load_feature_table)  # noqa: F401
