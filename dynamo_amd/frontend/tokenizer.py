"""Tokenizers for the frontend preprocessor.

ByteTokenizer: deterministic byte-level tokenizer (no network, no files) —
the default for synthetic/random-weight serving and tests.
HFTokenizer: wraps a local `tokenizers` JSON file when one exists.
Chat templating is jinja2 with a Llama-3-style default template
(the reference renders chat templates via minijinja —
preprocessor.rs OpenAIPreprocessor; ours is the Python analog).
"""
from __future__ import annotations

import codecs
from typing import List, Optional

import jinja2

_BYTE_ERRORS = "dynamo_amd_latin1"
_Utf8Stream = codecs.getincrementaldecoder("utf-8")


def _latin1_errors(exc):
    if not isinstance(exc, UnicodeDecodeError):
        raise exc
    return exc.object[exc.start:exc.end].decode("latin-1"), exc.end


codecs.register_error(_BYTE_ERRORS, _latin1_errors)

DEFAULT_CHAT_TEMPLATE = (
    "{% for m in messages %}"
    "<|start_header_id|>{{ m.role }}<|end_header_id|>\n\n{{ m.content }}<|eot_id|>"
    "{% endfor %}"
    "{% if add_generation_prompt %}"
    "<|start_header_id|>assistant<|end_header_id|>\n\n"
    "{% endif %}"
)


class ByteTokenizer:
    """Bytes + special tokens. ids: 0..255 = bytes; 256=bos, 257=eos,
    258=pad; vocab padded to `vocab_size`."""

    def __init__(self, vocab_size: int = 512):
        self.vocab_size = max(vocab_size, 260)
        self.bos_id = 256
        self.eos_id = 257
        self.pad_id = 258

    def encode(self, text: str, add_bos: bool = False) -> List[int]:
        ids = list(text.encode("utf-8"))
        return ([self.bos_id] if add_bos else []) + ids

    def decode(self, ids: List[int]) -> str:
        # Streaming-safe: the text of a prefix of `ids` is always a prefix
        # of the text of `ids`, whatever bytes follow. Valid UTF-8 decodes
        # as such; a byte that cannot be part of a valid sequence
        # (synthetic tokens) maps to its latin-1 char, which keeps distinct
        # bytes distinct (utf-8 replacement chars would collapse them); an
        # incomplete sequence at the very end is held back until the bytes
        # that complete or invalidate it arrive.
        bs = bytes(i for i in ids if 0 <= i < 256)
        return _Utf8Stream(_BYTE_ERRORS).decode(bs, False)

    def decode_incremental(self, ids: List[int], prev_len: int) -> str:
        """Text added by ids[prev_len:], robust to split UTF-8 sequences:
        concatenated chunks equal decode(ids) for any chunking."""
        return self.decode(ids)[len(self.decode(ids[:prev_len])):]


class HFTokenizer:
    def __init__(self, path: str):
        from tokenizers import Tokenizer
        self.tk = Tokenizer.from_file(path)
        self.vocab_size = self.tk.get_vocab_size()
        self.eos_id = None
        for cand in ("</s>", "<|eot_id|>", "<|endoftext|>", "<eos>"):
            tid = self.tk.token_to_id(cand)
            if tid is not None:
                self.eos_id = tid
                break
        self.bos_id = self.tk.token_to_id("<s>")

    def encode(self, text: str, add_bos: bool = False) -> List[int]:
        ids = self.tk.encode(text).ids
        return ([self.bos_id] if add_bos and self.bos_id is not None else []) + ids

    def decode(self, ids: List[int]) -> str:
        return self.tk.decode(ids)

    def decode_incremental(self, ids: List[int], prev_len: int) -> str:
        # decode with one token of left context to keep merges stable
        full = self.tk.decode(ids[max(0, prev_len - 1):])
        prevtxt = self.tk.decode(ids[max(0, prev_len - 1):prev_len])
        return full[len(prevtxt):]


def make_tokenizer(spec: Optional[dict]):
    spec = spec or {}
    t = spec.get("type", "byte")
    if t == "byte":
        return ByteTokenizer(spec.get("vocab_size", 512))
    if t == "hf":
        return HFTokenizer(spec["path"])
    raise ValueError(f"unknown tokenizer type {t!r}")


class ChatTemplater:
    def __init__(self, template: Optional[str] = None):
        self.env = jinja2.Environment()
        self.template = self.env.from_string(template or DEFAULT_CHAT_TEMPLATE)

    def render(self, messages: List[dict],
               add_generation_prompt: bool = True) -> str:
        return self.template.render(messages=messages,
                                    add_generation_prompt=add_generation_prompt)
