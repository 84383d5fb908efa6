"""The reference's abstract dataset (engine/utils/dataset/dataset.py): what a generator may ask of a dataset."""


class Dataset:
    def __init__(self, **kwargs):
        pass

    def __len__(self):
        raise NotImplementedError

    def __getitem__(self, index):
        raise NotImplementedError

    def shuffle(self):
        raise NotImplementedError

    def get_config(self):
        raise NotImplementedError
