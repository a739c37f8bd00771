"""Video retrieval command-line tools, named after the reference's scripts/ (extract_features,
build_index, query_video, eval_retrieval) and running on the HIP path (vcap.retrieval)."""
