from recbole_amd.model.general_recommender.bpr import BPR
from recbole_amd.model.general_recommender.lightgcn import LightGCN
from recbole_amd.model.general_recommender.neumf import NeuMF

__all__ = ['BPR', 'LightGCN', 'NeuMF']
