"""TEST INFRASTRUCTURE — what the ModernBERT cross-encoder tests share: a byte-level BPE tokenizer with the pair
template, and a synthetic one-label ModernBertForSequenceClassification directory of seeded weights."""
import json
import os

import numpy as np

import modernbert_oracle as mo
import modernbert_rerank_oracle as mro

WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth wavefront encoder "
         "attention window rotary position layer norm residual gate token chunk document search query score filter").split()


def bpe_pair_tokenizer(seed=61):
    """A byte-level BPE of ~400 pieces trained on WORDS, [CLS] $A [SEP] / [CLS] $A [SEP] $B [SEP]."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers

    tok = Tokenizer(models.BPE(unk_token=None))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=400, special_tokens=["[PAD]", "[CLS]", "[SEP]"], show_progress=False,
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    rng = np.random.default_rng(seed)
    tok.train_from_iterator([" ".join(rng.choice(WORDS, size=12)) + "." for _ in range(200)], trainer)
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                       special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    return tok


def reranker_checkpoint(d, pooling="mean", biases=False, seed=67, cls_scale=6.0, layers=3, max_length=128):
    """config.json (transformers 5's spelling), tokenizer.json, tokenizer_config.json and model.safetensors of a seeded
    ModernBertForSequenceClassification with one label -> (shape, weights, the tokenizers-library tokenizer)."""
    from safetensors.numpy import save_file

    os.makedirs(d, exist_ok=True)
    tok = bpe_pair_tokenizer()
    tok.save(os.path.join(d, "tokenizer.json"))
    vocab = -(-tok.get_vocab_size() // 8) * 8
    shape = mo.ModernShape(layers, 128, 2, 256, vocab=vocab, max_pos=8192, window=8)
    json.dump({"architectures": ["ModernBertForSequenceClassification"], "model_type": "modernbert", "hidden_size": 128,
               "num_hidden_layers": layers, "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": vocab,
               "max_position_embeddings": 8192, "norm_eps": shape.eps, "norm_bias": biases, "hidden_activation": "gelu",
               "local_attention": 16, "global_attn_every_n_layers": 3,
               "layer_types": ["full_attention" if i % 3 == 0 else "sliding_attention" for i in range(layers)],
               "rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": shape.theta},
                                   "sliding_attention": {"rope_type": "default", "rope_theta": shape.theta_local}},
               "classifier_pooling": pooling, "classifier_activation": "gelu", "classifier_bias": biases,
               "id2label": {"0": "LABEL_0"}}, open(os.path.join(d, "config.json"), "w"))
    json.dump({"model_max_length": max_length}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    w = mro.random_weights(shape, seed, biases, cls_scale)
    save_file({(k if k.startswith(("head.", "classifier.")) else "model." + k): np.ascontiguousarray(v) for k, v in w.items()},
              os.path.join(d, "model.safetensors"))
    return shape, w, tok
