"""UserDataLoader (mirror of recbole/data/dataloader/user_dataloader.py:21-62): the train
loader of the autoencoder models (MultiDAE, MultiVAE). A batch holds user ids only, every
user of the dataset once per epoch, the pad user 0 included, as the reference's
arange(user_num); the models read the users' interaction rows from the dataset's history
CSR. The per-epoch shuffle is the Interaction's torch.randperm on the CPU generator, the
draw the other loaders here make, so a seed gives one order."""
import torch

from recbole_amd.data.dataloader.abstract_dataloader import AbstractDataLoader
from recbole_amd.data.interaction import Interaction
from recbole_amd.utils import DataLoaderType, InputType


class UserDataLoader(AbstractDataLoader):
    dl_type = DataLoaderType.ORIGIN

    def __init__(self, config, dataset, batch_size=1, dl_format=InputType.POINTWISE,
                 shuffle=False):
        self.uid_field = dataset.uid_field
        self.user_list = Interaction({self.uid_field: torch.arange(dataset.user_num)})
        super().__init__(config, dataset, batch_size=batch_size, dl_format=dl_format,
                         shuffle=shuffle)

    def setup(self):
        if self.shuffle is False:
            self.shuffle = True
            self.logger.warning('UserDataLoader must shuffle the data')

    @property
    def pr_end(self):
        return len(self.user_list)

    def _shuffle(self):
        self.user_list.shuffle()

    def _next_batch_data(self):
        cur_data = self.user_list[self.pr:self.pr + self.step]
        self.pr += self.step
        return cur_data
