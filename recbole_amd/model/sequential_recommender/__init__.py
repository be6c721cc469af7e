from recbole_amd.model.sequential_recommender.bert4rec import BERT4Rec
from recbole_amd.model.sequential_recommender.gru4rec import GRU4Rec
from recbole_amd.model.sequential_recommender.sasrec import SASRec

__all__ = ['BERT4Rec', 'GRU4Rec', 'SASRec']
