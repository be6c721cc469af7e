from recbole_amd.model.general_recommender.bpr import BPR
from recbole_amd.model.general_recommender.lightgcn import LightGCN
from recbole_amd.model.general_recommender.multidae import MultiDAE
from recbole_amd.model.general_recommender.multivae import MultiVAE
from recbole_amd.model.general_recommender.neumf import NeuMF

__all__ = ['BPR', 'LightGCN', 'MultiDAE', 'MultiVAE', 'NeuMF']
