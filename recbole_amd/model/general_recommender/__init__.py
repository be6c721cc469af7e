from recbole_amd.model.general_recommender.bpr import BPR
from recbole_amd.model.general_recommender.lightgcn import LightGCN
from recbole_amd.model.general_recommender.multidae import MultiDAE
from recbole_amd.model.general_recommender.multivae import MultiVAE
from recbole_amd.model.general_recommender.neumf import NeuMF
from recbole_amd.model.general_recommender.ngcf import NGCF

__all__ = ['BPR', 'LightGCN', 'MultiDAE', 'MultiVAE', 'NGCF', 'NeuMF']
