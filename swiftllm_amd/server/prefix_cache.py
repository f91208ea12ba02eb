"""PrefixCache — which finished sequences still hold KV blocks a new prompt could reuse (pure host code, no torch).

Prefix caching here is reuse by COPY: a finished request keeps its block-table row and its blocks
as a cache entry; a new prompt whose leading whole blocks equal an entry's gets private copies of those blocks
(LlamaModel.copy_kv_prefix) and prefills only the rest. Nothing is shared, so this index only has to answer "which entry
has the longest common whole-block prefix with this prompt" and "which entry goes first".

It is a trie over whole blocks. A node is keyed, under its parent, by the exact tuple of a block's token ids — no hashes,
so no collisions — and holds the set of entries whose sequence contains that chain of blocks. Every node holds at least
one entry (an emptied node is deleted), and every entry of a child is an entry of its parent.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple


class CacheEntry:
    """One cached sequence: its block-table row, the KV blocks the row holds (all of them stay with it: what the scheduler
    counts), the tokens of its whole blocks (what a prompt may reuse) and its LRU stamp."""
    __slots__ = ("seq_id", "num_blocks_held", "num_cached_tokens", "last_use", "_keys")

    def __init__(self, seq_id: int, num_blocks_held: int, num_cached_tokens: int, last_use: int, keys: List[tuple]):
        self.seq_id = seq_id
        self.num_blocks_held = num_blocks_held
        self.num_cached_tokens = num_cached_tokens
        self.last_use = last_use
        self._keys = keys       # the block keys of its own path, root first

    def __repr__(self):
        return (f"CacheEntry(seq_id={self.seq_id}, num_blocks_held={self.num_blocks_held}, "
                f"num_cached_tokens={self.num_cached_tokens}, last_use={self.last_use})")


class _Node:
    __slots__ = ("children", "entries")

    def __init__(self):
        self.children: Dict[tuple, "_Node"] = {}
        self.entries: Set[CacheEntry] = set()


class PrefixCache:
    def __init__(self, block_size: int, max_entries: int):
        if block_size <= 0 or max_entries <= 0:
            raise ValueError("PrefixCache needs a positive block_size and max_entries")
        self.block_size = block_size
        self.max_entries = max_entries
        self._root = _Node()
        self._entries: Dict[int, CacheEntry] = {}       # seq id -> entry
        self._clock = 0
        self.num_blocks_held = 0        # over all entries

    def __len__(self) -> int:
        return len(self._entries)

    def entries(self) -> List[CacheEntry]:
        return list(self._entries.values())

    def _tick(self) -> int:
        self._clock += 1
        return self._clock

    def _block_keys(self, token_ids: Sequence[int], num_blocks: int) -> List[tuple]:
        bs = self.block_size
        return [tuple(token_ids[i * bs:(i + 1) * bs]) for i in range(num_blocks)]

    def _walk(self, keys: Iterable[tuple]) -> Tuple[_Node, int]:
        """The deepest node of the chain `keys` that exists, and its depth in blocks."""
        node, depth = self._root, 0
        for key in keys:
            child = node.children.get(key)
            if child is None:
                break
            node, depth = child, depth + 1
        return node, depth

    def match(self, prompt_ids: Sequence[int]) -> Tuple[Optional[CacheEntry], int]:
        """(entry, tokens): the entry sharing the longest chain of whole blocks with the prompt and the tokens of that
        chain, capped at ((len(prompt) - 1) // block_size) * block_size — at least one prompt token must be forwarded to
        get the first output token. Several entries at that depth: the most recently used. (None, 0): no block matches.
        A match touches the entry's LRU stamp."""
        cap = (len(prompt_ids) - 1) // self.block_size if len(prompt_ids) > 0 else 0
        node, depth = self._walk(self._block_keys(prompt_ids, cap))
        if depth == 0:
            return None, 0
        entry = max(node.entries, key=lambda e: e.last_use)
        entry.last_use = self._tick()
        return entry, depth * self.block_size

    def holds(self, token_ids: Sequence[int]) -> bool:
        """Some entry already contains every whole block of `token_ids` (inserting it would add nothing)."""
        nb = len(token_ids) // self.block_size
        return nb == 0 or self._walk(self._block_keys(token_ids, nb))[1] == nb

    def insert(self, seq_id: int, token_ids: Sequence[int], blocks_held: int) -> bool:
        """Register the whole blocks of `token_ids` as held by block-table row `seq_id` (which holds `blocks_held` KV
        blocks in all). False — the caller frees the row as it always did — when there is no whole block, when the deepest
        node of its chain already holds an entry (the same prompt twice adds nothing), when the row is already an entry,
        or when the cache is full (the caller evicts first)."""
        nb = len(token_ids) // self.block_size
        if nb == 0 or seq_id in self._entries or len(self._entries) >= self.max_entries:
            return False
        keys = self._block_keys(token_ids, nb)
        if self._walk(keys)[1] == nb:
            return False
        entry = CacheEntry(seq_id, int(blocks_held), nb * self.block_size, self._tick(), keys)
        node = self._root
        for key in keys:
            child = node.children.get(key)
            if child is None:
                child = node.children[key] = _Node()
            child.entries.add(entry)
            node = child
        self._entries[seq_id] = entry
        self.num_blocks_held += entry.num_blocks_held
        return True

    def _unlink(self, entry: CacheEntry):
        """Take the entry off every node of its own path; a node left without entries is deleted (its children are
        empty too: every entry of a child is an entry of its parent)."""
        node = self._root
        for key in entry._keys:
            child = node.children[key]
            child.entries.discard(entry)
            if not child.entries:
                del node.children[key]
                break
            node = child
        del self._entries[entry.seq_id]
        self.num_blocks_held -= entry.num_blocks_held

    def evict_lru(self, exclude: Iterable[int] = ()) -> Optional[CacheEntry]:
        """Remove and return the least recently used entry whose seq_id is not in `exclude`; None when there is none."""
        exclude = set(exclude)
        victim = min((e for e in self._entries.values() if e.seq_id not in exclude), key=lambda e: e.last_use,
                     default=None)
        if victim is not None:
            self._unlink(victim)
        return victim

    def clear(self) -> List[int]:
        """Forget everything; returns the seq ids of the entries (the caller frees their rows)."""
        ids = list(self._entries)
        self._root = _Node()
        self._entries = {}
        self.num_blocks_held = 0
        return ids
