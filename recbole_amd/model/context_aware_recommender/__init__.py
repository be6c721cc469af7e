from recbole_amd.model.context_aware_recommender.afm import AFM
from recbole_amd.model.context_aware_recommender.dcn import DCN
from recbole_amd.model.context_aware_recommender.deepfm import DeepFM
from recbole_amd.model.context_aware_recommender.xdeepfm import xDeepFM

__all__ = ['AFM', 'DCN', 'DeepFM', 'xDeepFM']
