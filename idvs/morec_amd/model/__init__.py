from .model import Model  # noqa: F401  (same import surface as the reference: ``from model import Model``)
from .encoders import ADD, CAT, Bert_Encoder, IdEmbedding, MAE_Encoder, Text_Encoder, Text_Encoder_mean, User_Encoder  # noqa: F401
from .bert import HipBertModel  # noqa: F401
from .spec import BertShape  # noqa: F401
from .beit import HipBeitForImageClassification  # noqa: F401
from .mae import HipViTMAEModel  # noqa: F401
from .opt import HipOPTModel  # noqa: F401
from ..opt_engine import OptShape  # noqa: F401
from .deberta import HipDebertaModel  # noqa: F401
from ..deberta_engine import DebertaShape  # noqa: F401
from .bce import BceModel  # noqa: F401  (drop-in for bce_text/main-end2end/model/model.py)
from .dssm import DssmModel, MLP_Encoder  # noqa: F401  (drop-in for bce_text/main-end2end(DSSM)/model/model.py)
from .two_stage import MLP_Layers, TwoStageModel  # noqa: F401  (drop-in for bce_text|bce_vision/main-2stage(SASRec)/model/model.py)
from .id_two_stage import FC_Layers, IdTwoStageModel, IdTwoStageModelVision  # noqa: F401  (drop-in for bce_text|bce_vision/id_plus_mo-2stage/model/model.py)
