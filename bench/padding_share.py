"""How much padding do the real data streams carry?  (CPU only; no model.)

For every batch a stream emits: the real tokens sum(len), the rows the rectangular path computes
on (B x the longest row rounded up to 64, models/albert.py encode) and the rows the packed path
computes on (sum of round_up(len, 64), data/packing.py).  Prints one JSON line per stream:

    python bench/padding_share.py --text README.md docs/*.md --batches 300 --batch 16 --seq 512

  * ``streaming``: StreamingSOPStream over the given local text files (paragraphs are documents),
    tokenized by a WordPiece model trained on the same files;
  * ``disk``: DiskSOPStream over a dataset built from the synthetic corpus of
    tests/test_sop_dataset.py (1-12 short sentences per document).
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dedloc_amd.data.packing import slot_rows  # noqa: E402
from dedloc_amd.data.sop_dataset import DiskSOPStream, StreamingSOPStream, build_dataset  # noqa: E402


def train_tokenizer(texts, vocab, out_dir):
    from tokenizers import Tokenizer, models, pre_tokenizers, processors, trainers
    from transformers import PreTrainedTokenizerFast

    tok = Tokenizer(models.WordPiece(unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.train_from_iterator(texts, trainers.WordPieceTrainer(
        vocab_size=vocab, special_tokens=["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]))
    cls, sep = tok.token_to_id("[CLS]"), tok.token_to_id("[SEP]")
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                       special_tokens=[("[CLS]", cls), ("[SEP]", sep)])
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]", pad_token="[PAD]", cls_token="[CLS]",
                                   sep_token="[SEP]", mask_token="[MASK]")
    fast.save_pretrained(out_dir)
    return fast


def measure(name, stream, batches, **info):
    real = padded = packed = 0
    lens_all = []
    for _ in range(batches):
        stream.next_batch()
        lens = stream.last_lengths
        B, L = len(lens), max(lens)
        real += sum(lens)
        padded += B * ((L + 63) // 64 * 64)
        packed += slot_rows(lens)[-1]
        lens_all += lens
    lens_all.sort()
    print(json.dumps({"stream": name, "batches": batches, **info,
                      "real_token_share_of_padded_rows": round(real / padded, 4),
                      "packed_rows_share_of_padded_rows": round(packed / padded, 4),
                      "real_token_share_of_packed_rows": round(real / packed, 4),
                      "len_min": lens_all[0], "len_median": lens_all[len(lens_all) // 2], "len_max": lens_all[-1]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", nargs="*", default=[], help="local text files for the streaming measurement")
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=2000)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if a.text:
            docs = []
            for p in a.text:
                with open(p, encoding="utf-8", errors="ignore") as f:
                    docs += [d.strip() for d in f.read().split("\n\n") if len(d.split()) > 3]
            src = os.path.join(tmp, "corpus.txt")
            with open(src, "w") as f:  # read_documents: blank-line separated documents
                f.write("\n\n".join(d.replace("\n", " ") for d in docs))
            tok = train_tokenizer(docs, a.vocab, os.path.join(tmp, "tok"))
            st = StreamingSOPStream([(src, 1.0)], tok, a.batch, seed=0, max_seq_length=a.seq, shuffle_buffer=1000)
            measure("streaming", st, a.batches, batch=a.batch, seq=a.seq, documents=len(docs), files=len(a.text))
        fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "test_sop_dataset.py")
        spec = importlib.util.spec_from_file_location("sop_fixture", fixture)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        docs = mod._corpus(400, seed=0)
        tok = train_tokenizer(mod._corpus(200, seed=1), 200, os.path.join(tmp, "tok2"))
        for seq in (64, a.seq):
            ds_dir = os.path.join(tmp, f"ds{seq}")
            build_dataset(docs, tok, ds_dir, max_seq_length=seq, seed=0)
            measure("disk", DiskSOPStream(ds_dir, a.batch, seed=0), a.batches, batch=a.batch, seq=seq, documents=len(docs))


if __name__ == "__main__":
    main()
