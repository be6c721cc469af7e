from recbole_amd.model.sequential_recommender.gru4rec import GRU4Rec
from recbole_amd.model.sequential_recommender.sasrec import SASRec

__all__ = ['GRU4Rec', 'SASRec']
