"""The builder / indexer interface of the retrieval stage (API mirror of torch_rechub/serving/base.py)."""
import abc


class BaseBuilder(abc.ABC):
    """Holds the build-time configuration of an index; ``from_embeddings`` and ``from_index_file`` are context managers
    that yield a ``BaseIndexer``:

    >>> with builder.from_embeddings(item_vectors) as indexer:
    ...     ids, values = indexer.query(user_vectors, top_k=10)
    ...     indexer.save("items.index")
    """

    @abc.abstractmethod
    def from_embeddings(self, embeddings):
        """Context manager yielding an indexer over the rows of ``embeddings`` (n, d)."""

    @abc.abstractmethod
    def from_index_file(self, index_file):
        """Context manager yielding the indexer that ``BaseIndexer.save`` wrote to ``index_file``."""


class BaseIndexer(abc.ABC):
    """A built index."""

    @abc.abstractmethod
    def query(self, embeddings, top_k):
        """(ids (n, top_k), distances (n, top_k)) of the ``top_k`` nearest rows for each row of ``embeddings`` (n, d),
        best first."""

    @abc.abstractmethod
    def save(self, file_path):
        """Write the index to ``file_path``."""
